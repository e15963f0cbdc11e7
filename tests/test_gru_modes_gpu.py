"""The two bf16 recurrence forms of the decoder's sizes (gru_resident_kernel, gru_mfma_kernel; H = 128 / 256) behind
their three doors: vc_gru_bidir with the form forced (packs on every call), vc_gru_pack + vc_gru_bidir_packed (packs
once), and modules._gru_recurrence / modules.gru, which choose the form by the makespan of the call (vc_gru_form) and
keep one packed image per (scope, form) in the variable store.

Expected values, inputs and bounds are those of the recurrent-kernel tests (tests/rnn_ref.py float64 definitions;
rnn_case / rnn_bound of tests/test_rnn_kernels_cpu.py: 4 x the bf16-state restatement's own distance from float64 on the
same input, at least 1e-6).  T = 5 throughout; n_seq 17 and 33 leave a ragged last 16-sequence MFMA workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_rnn_kernels_cpu import VC_BF16, VC_F32, rnn_bound, rnn_case

pytestmark = pytest.mark.gpu

RESIDENT, MFMA = 1, 2
FORM_OF = {0: RESIDENT, 1: MFMA}          # option gru_mfma -> form
T = 5
N_SEQ = (1, 16, 17, 33)


@pytest.fixture(autouse=True)
def _default_options():
    import _vc
    assert _vc.get_option('gru_mfma') == -1
    yield
    _vc.set_option('gru_mfma', -1)


def p(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().copy()


def _dev(c):
    return (torch.from_numpy(np.array(c['xproj'])).cuda(), torch.from_numpy(np.array(c['wf'])).bfloat16().cuda(),
            torch.from_numpy(np.array(c['wb'])).bfloat16().cuda())


def per_call(c, gm, out_dtype=VC_F32):
    """vc_gru_bidir with the form forced: the weights are packed into the workspace by this call."""
    import _vc
    lib = _vc.lib()
    H, n_seq = c['H'], c['n_seq']
    x, wf, wb = _dev(c)
    out = torch.full((n_seq * T, 2 * H), float('nan'), dtype=torch.float32 if out_dtype == VC_F32 else torch.bfloat16, device='cuda')
    need = int(lib.vc_gru_workspace_bytes(H, VC_BF16))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    with _vc.options(gru_mfma=gm):
        _vc.check(lib.vc_gru_bidir(p(x), p(wf), p(wb), VC_BF16, n_seq, T, H, p(out), out_dtype, p(ws), need, _vc.current_stream()))
    torch.cuda.synchronize()
    return out


def pre_packed(c, form, out_dtype=VC_F32):
    """vc_gru_pack once, then vc_gru_bidir_packed on the image (followed by a canary that must survive the packing)."""
    import _vc
    lib = _vc.lib()
    H, n_seq = c['H'], c['n_seq']
    x, wf, wb = _dev(c)
    need = int(lib.vc_gru_packed_bytes(form, H, VC_BF16))
    assert need == 2 * 3 * H * H * 2
    img = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device='cuda')
    _vc.check(lib.vc_gru_pack(form, p(wf), p(wb), VC_BF16, H, p(img), need, _vc.current_stream()))
    torch.cuda.synchronize()
    assert bool((img[need:] == 0xA5).all()), 'wrote past vc_gru_packed_bytes'
    del wf, wb                                                  # the run reads the image alone
    out = torch.full((n_seq * T + 1, 2 * H), float('nan'), dtype=torch.float32 if out_dtype == VC_F32 else torch.bfloat16, device='cuda')
    _vc.check(lib.vc_gru_bidir_packed(form, p(x), p(img), need, VC_BF16, n_seq, T, H, p(out), out_dtype, _vc.current_stream()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n_seq * T:].float()).all()), 'wrote past the last row'
    return out[:n_seq * T]


def _within_bound(got, c, what, out_dtype=VC_F32):
    H = c['H']
    bound, cap = rnn_bound(c, True, out_dtype)
    assert float(bound.max()) <= cap
    got = got.double().cpu().numpy()
    err = np.abs(got - c['want'])
    for name, sl in (('forward', slice(0, H)), ('backward', slice(H, 2 * H))):
        e, b = float(err[:, sl].max()), float(bound[:, sl].max())
        print('MEASURED %s H=%d n_seq=%d %s err=%.2e bound=%.2e' % (what, H, c['n_seq'], name, e, b))
        assert np.isfinite(got[:, sl]).all() and bool((err[:, sl] <= bound[:, sl]).all()), (what, H, c['n_seq'], name, e, b)


@pytest.mark.parametrize('n_seq', N_SEQ)
@pytest.mark.parametrize('H', [128, 256])
def test_both_forms_against_float64_and_packed_once_equals_packed_per_call(H, n_seq):
    """Each form forced (gru_mfma = 0 / 1), both directions, against the float64 recurrence; the same form on an image
    packed once gives the same bits, float32 and bf16 output; the two forms differ from each other (so 'the same bits'
    says which kernel ran)."""
    c = rnn_case('gru', H, T, n_seq, VC_BF16)
    res = {}
    for gm in (0, 1):
        res[gm] = per_call(c, gm)
        _within_bound(res[gm], c, 'forced gru_mfma=%d' % gm)
        once = pre_packed(c, FORM_OF[gm])
        _within_bound(once, c, 'packed once, form %d' % FORM_OF[gm])
        assert np.array_equal(bits(once), bits(res[gm])), (H, n_seq, gm, 'packed once differs from packed per call')
        assert np.array_equal(bits(pre_packed(c, FORM_OF[gm], VC_BF16)), bits(per_call(c, gm, VC_BF16))), (H, n_seq, gm, 'bf16 output')
    assert not np.array_equal(bits(res[0]), bits(res[1])), 'the two forms cannot be told apart on this input'


def _recurrence(store, c, scope):
    import modules
    x, wf, wb = _dev(c)
    with modules.variable_store(store):
        y = modules._gru_recurrence(x, c['n_seq'], T, c['H'], wf, wb, scope=scope)
    torch.cuda.synchronize()
    return y.reshape(c['n_seq'] * T, 2 * c['H'])


def test_auto_takes_the_resident_form_in_one_round_of_cus_and_mfma_in_throughput_mode():
    """256 units: 33 sequences are 66 resident workgroups, one round of CUs on any device of 66 CUs or more (an MI355X has
    256), so the default is the resident form, bit for bit; under _vc.throughput_mode() it is the MFMA form."""
    import _vc
    import modules
    H, n_seq = 256, 33
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lib = _vc.lib()
    want_gm = 0 if 2 * n_seq <= n_cu else 1
    assert lib.vc_gru_form(H, VC_BF16, n_seq, 0) == lib.vc_gru_form(H, VC_BF16, n_seq, n_cu) == FORM_OF[want_gm]
    assert lib.vc_gru_form(H, VC_BF16, n_cu // 2 + 1, 0) == MFMA and lib.vc_gru_form(H, VC_BF16, n_cu // 2, 0) == RESIDENT
    c = rnn_case('gru', H, T, n_seq, VC_BF16)
    forced = {gm: bits(per_call(c, gm, VC_BF16)) for gm in (0, 1)}
    assert not np.array_equal(forced[0], forced[1])
    st = modules.VariableStore('bfloat16')
    assert np.array_equal(bits(_recurrence(st, c, 'auto')), forced[want_gm]), 'default is not the form the rule names'
    with _vc.throughput_mode():
        assert np.array_equal(bits(_recurrence(st, c, 'auto')), forced[1]), 'throughput mode did not take the MFMA form'
    assert _vc.get_option('gru_mfma') == -1
    assert np.array_equal(bits(_recurrence(st, c, 'auto')), forced[want_gm])


def test_auto_at_128_units_keeps_its_threshold():
    """128 units: the two forms take the same time alone at 64 sequences (profiles/gru_modes/README.md), so the default
    stays what it was: resident at 17 sequences, MFMA at 33, and MFMA at both under _vc.throughput_mode()."""
    import _vc
    import modules
    for n_seq, want_gm in ((17, 0), (33, 1)):
        st = modules.VariableStore('bfloat16')                   # (a store per case: the cases' weights differ)
        c = rnn_case('gru', 128, T, n_seq, VC_BF16)
        forced = {gm: bits(per_call(c, gm, VC_BF16)) for gm in (0, 1)}
        assert not np.array_equal(forced[0], forced[1])
        assert np.array_equal(bits(_recurrence(st, c, 'auto128')), forced[want_gm]), n_seq
        with _vc.throughput_mode():
            assert np.array_equal(bits(_recurrence(st, c, 'auto128')), forced[1]), n_seq


@pytest.mark.parametrize('H', [128, 256])
def test_switching_the_mode_on_one_store_gives_each_form_its_own_image(H):
    """The two kernels read different layouts: the cached image is keyed by the form, so 0 -> 1 -> 0 -> 1 on one store and
    one scope gives each form's own result every time (the other form's image would give garbage, not a small error)."""
    import _vc
    import modules
    c = rnn_case('gru', H, T, 17, VC_BF16)
    forced = {gm: bits(per_call(c, gm, VC_BF16)) for gm in (0, 1)}
    st = modules.VariableStore('bfloat16')
    for gm in (0, 1, 0, 1, 1, 0):
        with _vc.options(gru_mfma=gm):
            y = _recurrence(st, c, 'sw')
        assert np.array_equal(bits(y), forced[gm]), (H, gm)
        _within_bound(y, c, 'one store, gru_mfma=%d' % gm, VC_BF16)
    keys = [k for k in st._cache if k[0] == 'gru_rec_pk']
    assert sorted(k[2] for k in keys) == [RESIDENT, MFMA] and all(k[1] == 'sw' for k in keys)
    st.invalidate()
    assert not [k for k in st._cache if k[0] == 'gru_rec_pk']


@pytest.mark.parametrize('gm', [0, 1])
@pytest.mark.parametrize('H', [128, 256])
def test_changed_recurrent_weights_are_repacked_after_invalidate(H, gm):
    """store.assign of a recurrent kernel + store.invalidate(): the next call equals a fresh store holding the new
    weights, and differs from the call before the change (a stale image would repeat it)."""
    import _vc
    import modules
    rng = np.random.RandomState(H + gm)
    N = 3
    x = modules.convert(torch.from_numpy((0.7 * rng.standard_normal((N, T, H))).astype(np.float32)).cuda(), torch.bfloat16)

    def run(store):
        with _vc.options(gru_mfma=gm), modules.variable_store(store), modules.variable_scope('g'):
            y = modules.gru(x, num_units=H, bidirection=True)
        torch.cuda.synchronize()
        return bits(y)

    st = modules.VariableStore('bfloat16', seed=1)
    before = run(st)
    assert np.array_equal(run(st), before)                      # second call: the cached image
    for d in ('fw', 'bw'):
        name = 'g/gru/bidirectional_rnn/%s/gru_cell/candidate/kernel' % d
        w = st.vars[name].clone()
        w[H:] = w[H:].flip(0) * 0.5                             # the recurrent rows only (rows [0, cin) multiply x)
        st.assign(name, w)
    st.invalidate()
    after = run(st)
    fresh = modules.VariableStore('bfloat16', seed=2)
    run(fresh)                                                  # creates the variables (other values)
    fresh.load_dict(st.to_numpy())
    assert np.array_equal(after, run(fresh)), 'not the result of the new weights'
    assert not np.array_equal(after, before), 'the change of the recurrent weights did not reach the kernel'
