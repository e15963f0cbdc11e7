"""The host side of the two bf16 recurrence forms (csrc/vc_rnn.hip: gru_pick_form behind vc_gru_form, the packed-image
entry points' argument checks, _vc.throughput_mode()), without a device: vc_gru_form is pure host code when it is given
a CU count, and the packed entry points refuse bad arguments before any HIP call."""
import pytest

VC_F32, VC_BF16 = 0, 1
NONE, RESIDENT, MFMA = 0, 1, 2
VC_ERR_INVALID, VC_ERR_WORKSPACE = 1, 3


@pytest.fixture(autouse=True)
def _default_options():
    import _vc
    assert _vc.get_option('gru_mfma') == -1
    yield
    _vc.set_option('gru_mfma', -1)


def _want(H, n_seq, n_cu):
    """The rule.  256 units: the resident form's grid of 2 n_seq workgroups in ONE round of the device's CUs, else the
    MFMA form.  128 units (the forms tie at 64 sequences): resident below 32 sequences, whatever the device."""
    if H == 128:
        return RESIDENT if n_seq < 32 else MFMA
    return RESIDENT if 2 * n_seq <= n_cu else MFMA


@pytest.mark.parametrize('n_cu', [1, 64, 256])
def test_form_follows_the_makespan_rule(n_cu):
    import _vc
    lib = _vc.lib()
    assert (_vc.GRU_FORM_NONE, _vc.GRU_FORM_RESIDENT, _vc.GRU_FORM_MFMA) == (NONE, RESIDENT, MFMA)
    for H in (128, 256):
        for n_seq in (1, 16, 17, 31, 32, 33, 64, 127, 128, 129, 1000, 2 ** 30):
            assert lib.vc_gru_form(H, VC_BF16, n_seq, n_cu) == _want(H, n_seq, n_cu), (H, n_seq, n_cu)
    # both sides of the edge, by hand
    edge = {1: (None, 1), 64: (32, 33), 256: (128, 129)}[n_cu]
    if edge[0] is not None:
        assert lib.vc_gru_form(256, VC_BF16, edge[0], n_cu) == RESIDENT
    assert lib.vc_gru_form(256, VC_BF16, edge[1], n_cu) == MFMA
    assert lib.vc_gru_form(128, VC_BF16, 31, n_cu) == RESIDENT and lib.vc_gru_form(128, VC_BF16, 32, n_cu) == MFMA
    assert lib.vc_gru_form(128, VC_BF16, 31, 0) == RESIDENT            # 128 units: no CU count, so no device needed
    # one CU never holds both directions of a 256-unit sequence: always the MFMA form
    assert n_cu != 1 or lib.vc_gru_form(256, VC_BF16, 1, 1) == MFMA


def test_the_option_forces_either_form_and_throughput_mode_pins_mfma():
    import _vc
    lib = _vc.lib()
    for n_cu in (1, 64, 256):
        for n_seq in (1, 33, 500):
            with _vc.options(gru_mfma=0):
                assert lib.vc_gru_form(256, VC_BF16, n_seq, n_cu) == RESIDENT
            with _vc.options(gru_mfma=1):
                assert lib.vc_gru_form(128, VC_BF16, n_seq, n_cu) == MFMA
            with _vc.throughput_mode():
                assert _vc.get_option('gru_mfma') == 1 and lib.vc_gru_form(256, VC_BF16, n_seq, n_cu) == MFMA
            assert _vc.get_option('gru_mfma') == -1
    # a forced form needs no CU count (and so no device)
    with _vc.options(gru_mfma=1):
        assert lib.vc_gru_form(256, VC_BF16, 64, 0) == MFMA


def test_sizes_without_a_packed_form():
    import _vc
    lib = _vc.lib()
    for H, dt in ((40, VC_BF16), (40, VC_F32), (128, VC_F32), (256, VC_F32), (129, VC_BF16), (512, VC_BF16), (0, VC_BF16), (256, 2)):
        for gm in (-1, 0, 1):
            _vc.set_option('gru_mfma', gm)
            assert lib.vc_gru_form(H, dt, 4, 256) == NONE and lib.vc_gru_form(H, dt, 4, 0) == NONE, (H, dt, gm)
        for form in (RESIDENT, MFMA):
            assert lib.vc_gru_packed_bytes(form, H, dt) == 0
    assert lib.vc_gru_form(256, VC_BF16, 0, 256) == NONE and lib.vc_gru_form(256, VC_BF16, -3, 256) == NONE
    for H in (128, 256):
        for form in (RESIDENT, MFMA):
            assert lib.vc_gru_packed_bytes(form, H, VC_BF16) == 2 * 3 * H * H * 2 == lib.vc_gru_workspace_bytes(H, VC_BF16)
        assert lib.vc_gru_packed_bytes(NONE, H, VC_BF16) == 0 and lib.vc_gru_packed_bytes(3, H, VC_BF16) == 0


def test_packed_entry_points_validate_before_any_launch():
    import _vc
    lib = _vc.lib()
    p = 4096                                      # any non-NULL address: never dereferenced
    need = 2 * 3 * 256 * 256 * 2
    assert lib.vc_gru_pack(RESIDENT, None, p, VC_BF16, 256, p, need, None) == VC_ERR_INVALID
    assert lib.vc_gru_pack(NONE, p, p, VC_BF16, 256, p, need, None) == VC_ERR_INVALID
    assert lib.vc_gru_pack(MFMA, p, p, VC_F32, 128, p, need, None) == VC_ERR_INVALID
    assert lib.vc_gru_pack(MFMA, p, p, VC_BF16, 40, p, need, None) == VC_ERR_INVALID
    assert lib.vc_gru_pack(MFMA, p, p, VC_BF16, 256, p, need - 1, None) == VC_ERR_WORKSPACE
    assert b'too small' in lib.vc_last_error()
    assert lib.vc_gru_bidir_packed(RESIDENT, p, None, need, VC_BF16, 1, 1, 256, p, VC_F32, None) == VC_ERR_INVALID
    assert lib.vc_gru_bidir_packed(3, p, p, need, VC_BF16, 1, 1, 256, p, VC_F32, None) == VC_ERR_INVALID
    assert lib.vc_gru_bidir_packed(MFMA, p, p, need, VC_BF16, 0, 1, 256, p, VC_F32, None) == VC_ERR_INVALID
    assert lib.vc_gru_bidir_packed(MFMA, p, p, need, VC_BF16, 1, 0, 256, p, VC_F32, None) == VC_ERR_INVALID
    assert lib.vc_gru_bidir_packed(MFMA, p, p, need, VC_BF16, 1, 1, 64, p, VC_F32, None) == VC_ERR_INVALID
    assert lib.vc_gru_bidir_packed(MFMA, p, p, need, VC_BF16, 1, 1, 256, p, 2, None) == VC_ERR_INVALID
    assert lib.vc_gru_bidir_packed(RESIDENT, p, p, need - 1, VC_BF16, 1, 1, 256, p, VC_F32, None) == VC_ERR_WORKSPACE
    assert lib.vc_gru_pack(MFMA, p, p, VC_BF16, 256, p + 8, need, None) == VC_ERR_INVALID               # 16-byte alignment of the image
    assert lib.vc_gru_bidir_packed(MFMA, p, p + 2, need, VC_BF16, 1, 1, 256, p, VC_F32, None) == VC_ERR_INVALID
