/* vc_hip.h -- C ABI of libvc_hip.so, the MI355X (gfx950) kernels behind the voice-conversion
 * hot path of socom20/speech-cloner.
 *
 * The reference has no FFI: its boundary is the Python construct-and-run API
 * (audio_lib.calc_MFCC_input, encoder.encoder_spec_phn, decoder.decoder_specs), whose
 * arithmetic lives in librosa/scipy/TensorFlow-1.9 ops.  Each entry point below replaces the
 * third-party op(s) one reference call site lowers to; the citation is the reference file:line.
 * The Python modules in speech-cloner_amd/ (same names as the reference's) bind these with
 * ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory (hipMalloc / torch.cuda tensor data_ptr);
 *     pointers named h_* are host memory; plain sizes are element counts unless "_bytes".
 *   - `stream` is a hipStream_t passed as void*; no entry point synchronises the stream or
 *     allocates device memory except the create / destroy calls, so every launch call is
 *     hipGraph-capturable.
 *   - return value: 0 = VC_OK, otherwise a VC_ERR_* code; vc_last_error() gives the message of
 *     the calling thread's last failure.  Nothing throws across the boundary.
 *   - tensors are row-major; activations are [N, T, C] (time-major inside a window, channels
 *     contiguous) exactly as the reference's TF tensors.
 */
#ifndef VC_HIP_H
#define VC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC_OK 0
#define VC_ERR_INVALID 1      /* bad argument (shape, null pointer, unsupported size) */
#define VC_ERR_HIP 2          /* a HIP runtime call failed */
#define VC_ERR_WORKSPACE 3    /* workspace too small */
#define VC_ERR_UNSUPPORTED 4

/* 2: vc_frontend_f32 / vc_frontend_stages_f32 take out_rows, vc_transpose_pad takes slack_row, vc_gemm_desc has
 *    sum_groups.  Bump on EVERY change of an exported signature or struct layout: the Python binding (_vc.py) refuses
 *    to load a library whose vc_version() differs from its own constant.  An export that is only added or removed
 *    (vc_ablate_build was the last one removed) does not bump it: the binding resolves every export by name at load.
 * 3: vc_gemm_desc ends with d_workspace / workspace_bytes (vc_conv_gemm_workspace_bytes); vc_bn_post_routing added.
 * 4: vc_split16 / vc_weights16 / vc_gemm16 (training convolutions on split-float16 operands).
 * 5: vc_mx8_quantize / vc_mx8_conv / vc_mx8_conv_workspace_bytes and vc_mx8_conv_desc (MX-FP8 inference).
 * 6: vc_griffin_lim_momentum_f32 / vc_vocoder_workspace_bytes_momentum (fast Griffin-Lim).
 * 7: vc_cut_windows / vc_compound_stitch / vc_phase_init (device-resident batched conversion). */
#define VC_ABI_VERSION 7

int vc_version(void);
const char* vc_last_error(void);
/* Name of the gfx target the code object was built for ("gfx950"). */
const char* vc_target_arch(void);

/* Kernel-selection options.  The library never reads the process environment; the only way to steer which of
 * two equivalent HIP kernels a launch takes (A/B measurements, regression tests) is this call.  Values: -1 = the
 * library's own choice (default).  Names:
 *   "bank256"        0 = filter banks on conv_kernel instead of bank256_kernel
 *   "bank256_xcd"    0 = plain 2-D grid, 1 = whole filter-width pairs per XCD, 2 = pairs split over two XCDs
 *   "conv256"        0 = long-K single filters on conv_kernel / gemm_kernel
 *   "conv256_min_k"  shortest K that takes conv256_kernel (default 384)
 *   "conv256_wm"     2 = keep 128-row blocks for 128-column launches
 *   "proj256"        0 = the 256-channel k = 3 projection on conv256_kernel instead of the bank tiles
 *   "proj256_split"  0 = never split that projection's K over two workgroups per row tile (see d_workspace)
 *   "wgrad_xcd"      0 = weight-gradient tiles dealt round-robin to the XCDs
 *   "gru_mfma"       0 = VALU (register-resident) recurrence always, 1 = MFMA recurrence always (default: vc_gru_bidir takes
 *                    the MFMA form from 32 sequences up; vc_gru_form at 256 units takes it when the resident grid exceeds one round of CUs)
 *   "fe_fused"       0 = the shipped front-end configuration as two launches (statistics pass, feature pass) instead of ONE
 *                    (every frame transformed once; blocks wait for the summary of their own utterance)
 *   "fe_fused_spin"  polls a block of the one-launch front-end waits for the other tiles of its utterance before it
 *                    computes their records itself (default 4000, ~4 ms); 0 = never wait (tests of that path)
 *   "prenet_lds"     0 = every wave of the fused prenet streams the weights from L2 itself (default: one stream per
 *                    block, shared through LDS)
 *   "gru_train_resident" 0 = the float32 training recurrences stream all their weights from L2 every step (default:
 *                    128 units: all of them in registers, forward and backward; 256 units: half, forward)
 *   "cbhg_front_mi"  4 = 128-row blocks in the fused encoder front
 *   "f32_f16x3"      0 = float32 INFERENCE keeps its filter banks / post-bank projections on the f32-input MFMA kernels
 *                    (default: three float16 products of exactly split operands, vc_gemm16: float32-accurate)
 *   "gru_f32_wide"   0 = float32 INFERENCE recurrences of more than 128 units stay on the streaming kernel (default: the
 *                    training forward kernel, which keeps half of the 786 KB of weights resident: 15.8 -> 3.0 ms at 64 windows)
 *   "gemm16_split"   vc_gemm16, single-pair launches: ways K is split over workgroups (1..8) + 16 * block map (0 = the splits
 *                    of a row tile on one XCD, 1 = one K range per XCD: ways must divide 8); default: chosen from the shape
 * Any other name is an unknown option and returns VC_ERR_INVALID.  That includes the two names that used to select the
 * four-wave MFMA recurrence and the encoder's 16-sequences-per-wave MFMA recurrence: both kernels were measured slower
 * and removed together with their options.  It also includes "ablate_bank256",
 * "ablate_bank256_only" and "ablate_cbhg_front", which skipped parts of a kernel for timing in a separate build of the
 * library: that build and every path it compiled in are gone, its measurements are in DESIGN.md sections 6 and 8.
 * All alternatives compute the same function (tests compare them).  Options are process-global; set them between launches.
 * They are read when a launch call is made, so a captured graph keeps the values of its capture: setting an option
 * afterwards does not change what the graph replays. */
int vc_set_option(const char* name, int value);
int vc_get_option(const char* name, int* value);

/* ------------------------------------------------------------------------------------------
 * Signal front-end: audio_lib.calc_MFCC_input  (/root/reference/audio_lib.py:89-244)
 *   amplitude normalisation (:125-126) -> pre-emphasis FIR (:12-28,:129-133) -> centred,
 *   reflect-padded STFT (:141-147, librosa.core.stft) -> |.|^2 -> power_to_db (:155-157) ->
 *   Slaney mel filterbank (:160-169) -> amplitude_to_db of the mel power (:172) -> DCT-II
 *   (:176-179) -> first-coefficient / scale / delta / min-shift / clip post-processing
 *   (:207-240), float32 time-major outputs (:244).
 * ------------------------------------------------------------------------------------------ */
typedef struct vc_frontend_cfg {
    int32_t sample_rate;               /* sr                       (default 16000) */
    int32_t hop_length;                /* hop_length                               */
    int32_t win_length;                /* win_length                               */
    int32_t n_fft;                     /* n_fft (None in Python -> win_length)     */
    int32_t n_mels;                    /* n_mels                                   */
    int32_t n_mfcc;                    /* n_mfcc                                   */
    float pre_emphasis;                /* 0.0 => filter skipped (audio_lib.py:129) */
    float mean_abs_amp_norm;           /* 1.0 => skipped        (audio_lib.py:125) */
    float mfcc_norm_factor;            /* 1.0 => skipped        (audio_lib.py:223) */
    float M_dB_norm_factor;            /* 1.0 => skipped        (audio_lib.py:234) */
    float P_dB_norm_factor;            /* 1.0 => skipped        (audio_lib.py:230) */
    int32_t mfcc_normaleze_first_mfcc; /* bool                  (audio_lib.py:220) */
    int32_t calc_mfcc_derivate;        /* bool                  (audio_lib.py:226) */
    int32_t clip_output;               /* bool                  (audio_lib.py:237) */
} vc_frontend_cfg;

typedef struct vc_frontend_plan vc_frontend_plan;

/* Host-only: the float64 tables a plan is built from, without touching the GPU.
 * h_mel [n_mels, 1+n_fft/2] = librosa.filters.mel(sr, n_fft, n_mels, norm=1) (audio_lib.py:160-166),
 * h_dct [n_mfcc, n_mels]    = librosa.filters.dct(n_mfcc, n_mels)            (audio_lib.py:176).
 * Either pointer may be NULL. */
int vc_frontend_host_tables(const vc_frontend_cfg* cfg, double* h_mel, double* h_dct);

/* Builds the device-side constant tables (window, DFT twiddles, sparse mel filterbank, DCT
 * basis).  h_window: host float64[win_length] analysis window (what
 * scipy.signal.get_window(name, win_length, fftbins=True) returns), or NULL for periodic hann.
 * Synchronous (small H2D copies). */
int vc_frontend_plan_create(const vc_frontend_cfg* cfg, const double* h_window,
                            vc_frontend_plan** out_plan);
void vc_frontend_plan_destroy(vc_frontend_plan* plan);

/* Number of frames for an L-sample utterance: 1 + L / hop_length  (audio_lib.py:52). */
int32_t vc_frontend_num_frames(const vc_frontend_plan* plan, int32_t n_samples);
/* Output feature widths: MFCC = n_mfcc * (1 | 2), mel = n_mels, power = 1 + n_fft/2. */
int32_t vc_frontend_mfcc_width(const vc_frontend_plan* plan);
int32_t vc_frontend_power_width(const vc_frontend_plan* plan);
/* Copies the dense float64 mel matrix [n_mels, 1+n_fft/2] / DCT basis [n_mfcc, n_mels] the
 * plan was built from into host buffers (for inspection and tests). */
int vc_frontend_get_mel(const vc_frontend_plan* plan, double* h_out);
int vc_frontend_get_dct(const vc_frontend_plan* plan, double* h_out);

size_t vc_frontend_workspace_bytes(const vc_frontend_plan* plan, int32_t batch, int32_t max_samples);

/* Batched feature extraction.
 *   d_wav      float32 [batch, wav_stride]   (utterance b = row b, first lens[b] samples)
 *   d_lens     int32   [batch] sample counts, or NULL => every utterance has max_samples
 *              (each must satisfy n_fft/2 < len <= max_samples)
 *   max_frames = 1 + max_samples / hop_length
 *   out_rows   row count of the outputs per utterance: 0 = max_frames; a smaller value stores only the first out_rows
 *              frames (the later ones still count for the utterance's normalisation statistics, as in the reference,
 *              which computes the whole utterance and then cuts windows: /root/reference/test.py:121-123, 240-241) -- e.g.
 *              800 for 4 s at hop 80, so that [batch, 800, n_mels] IS the [2 * batch, 400, n_mels] window batch of the
 *              encoder without a copy.  Needs the shipped configuration (either of its forms) when < max_frames.
 *   d_mfcc     float32 [batch, out_rows, mfcc_width]
 *   d_mel_db   float32 [batch, out_rows, n_mels]
 *   d_pow_db   float32 [batch, out_rows, 1 + n_fft/2]
 *              rows f >= 1 + lens[b]/hop of utterance b are zero-filled.
 *   d_workspace / workspace_bytes: scratch of at least vc_frontend_workspace_bytes(), owned by this call until it
 *              completes on `stream`: concurrent calls of one plan need separate workspaces.  The plan itself is
 *              read-only after vc_frontend_plan_create.
 * Shipped configuration (n_fft 400, hop 80, 80 mels, 40 cepstra): by default ONE launch (fe400_fused_kernel), preceded
 * on `stream` by a small kernel that zeroes the per-utterance arrival counters at the start of the workspace (a node of
 * its own under graph capture, replayed before the main one); with vc_set_option("fe_fused", 0) two launches, a
 * statistics pass and a feature pass.  Other configurations: STFT power + mel + raw dB with per-tile max / min / sum|x|
 * partials, then finalize (amplitude normalisation as a dB offset, amin and top_db clips, min shift, DCT, delta, clip);
 * with hop_length > n_fft/2 a third launch computes the per-utterance sum|x| first.  These launches keep their tiles in
 * up to 160 KB of dynamic LDS (all of them opted in above 64 KB); a configuration that vc_frontend_plan_create accepts
 * but whose tile would need more (very large n_mels x n_mfcc, hop_length in the thousands) is refused here with an error
 * that names the launch and its byte count. */
int vc_frontend_f32(const vc_frontend_plan* plan, const float* d_wav, const int32_t* d_lens,
                    int32_t batch, int32_t max_samples, int32_t wav_stride, int32_t out_rows,
                    float* d_mfcc, float* d_mel_db, float* d_pow_db,
                    void* d_workspace, size_t workspace_bytes, void* stream);

/* Same call restricted to a subset of its launches (measurement hook used by bench.py to time
 * one kernel with HIP events): stage_mask bit0 = |x| partial sums (a launch only when
 * hop_length > n_fft/2), bit1 = STFT power/mel/dB, bit2 = finalize.  Later stages read what earlier ones left in the workspace. */
int vc_frontend_stages_f32(const vc_frontend_plan* plan, const float* d_wav, const int32_t* d_lens,
                           int32_t batch, int32_t max_samples, int32_t wav_stride, int32_t out_rows,
                           float* d_mfcc, float* d_mel_db, float* d_pow_db,
                           void* d_workspace, size_t workspace_bytes, void* stream,
                           int32_t stage_mask);

/* ------------------------------------------------------------------------------------------
 * Network blocks: modules.py (/root/reference/modules.py:39-356) lowered to four kernels.
 * dtype codes for activations/weights: */
#define VC_F32 0
#define VC_BF16 1
/* activation codes */
#define VC_ACT_NONE 0
#define VC_ACT_RELU 1
#define VC_ACT_SIGMOID 2
#define VC_ACT_TANH 3
/* vc_gemm_desc.mode */
#define VC_GEMM_PLAIN 0
#define VC_GEMM_HIGHWAY 1
#define VC_GEMM_MAX_GROUPS 32

/* One implicit-GEMM launch:  C[m, c_off + n] = epilogue( sum_kk A[m, kk] * Bt[n, kk] ).
 *
 * A is a Toeplitz VIEW of the activation tensor X [M = N_windows*T rows, Cin channels, row
 * stride ldx]:  A[m, j*Cin + c] = X[m + j - pad_l, c]  if 0 <= (m mod T) + j - pad_l < T else 0,
 * which is exactly tf.layers.conv1d(padding="SAME", stride 1, no bias) on [N,T,Cin] with a
 * kernel stored [taps, Cin, Cout] (modules.py:104-140; pad_l = (taps-1)/2).  taps = 1 gives
 * tf.layers.dense (modules.py:291-293, 315-317; encoder.py:109; decoder.py:127,179).
 * Bt is the kernel TRANSPOSED to [Cout, taps*Cin] (K contiguous), dtype = `dtype`.
 *
 * Grouped launch (n_groups > 1) = conv1d_banks (modules.py:144-166): group g has its own
 * taps/pad_l/K/Bt and writes columns [c_off, c_off + N) of the shared output (the concat).
 *
 * Optional prologue on A (applied per element, in this order):
 *   pro_scale/pro_shift [Cin] affine, pro_relu, pro_pool: max(A[r], A[r+1]) along time with the
 *   TF "same" rule out[T-1] = x[T-1]  (tf.layers.max_pooling1d(2,1,"same"), modules.py:331);
 *   pro_pool = 2 additionally promises the values that are pooled (after affine / relu) are >= 0: the maximum is then
 *   taken on the bit patterns as SIGNED integers.  Accepted: +0.0, -0.0, every positive finite value and +inf; -0.0
 *   orders below all of them, so max(-0.0, x) = x and the result is a zero only where both frames are zeros (of either
 *   sign).  A negative value or a NaN breaks the promise (the result is then unspecified, as before).  pro_relu != 0
 *   selects the same maximum, whatever sign of zero the ReLU produced.
 *   The padding zeros of the Toeplitz view are inserted AFTER the prologue: a padding frame contributes 0, not pro_shift.
 * Epilogue: v = acc * epi_scale[c] + epi_shift[c] (NULL scale = 1, NULL shift = 0; this is the
 *   dense bias or the folded inference FusedBatchNorm of modules.py:39-102), activation,
 *   + residual R[m, n] (modules.py:340), stored as float32 (out_f32 != 0) or as `dtype`.
 * mode VC_GEMM_HIGHWAY (modules.py:297-319): Bt holds [32 rows of dense1^T | 32 rows of
 *   dense2^T] interleaved per 32 output units (N = 64*ceil(H/32) rows, zero-padded), epi_shift
 *   the biases in the same order; output [M, H]: relu(h)*sig(t) + x*(1 - sig(t)), x = X.
 * All device pointers; scale/shift vectors are float32. */
typedef struct vc_gemm_group {
    const void* d_Bt;   /* [N, K] transposed kernel, row stride K */
    int32_t K;          /* taps * Cin (multiple of 4 for f32, 8 for bf16) */
    int32_t taps;
    int32_t pad_l;
    int32_t c_off;      /* first output column of this group */
} vc_gemm_group;

typedef struct vc_gemm_desc {
    int32_t dtype;              /* VC_F32 | VC_BF16: type of X, Bt, R (and C unless out_f32) */
    int32_t mode;               /* VC_GEMM_PLAIN | VC_GEMM_HIGHWAY */
    const void* d_X;
    int32_t M, T, Cin, ldx;
    int32_t N;                  /* output columns per group */
    int32_t n_groups;
    vc_gemm_group groups[VC_GEMM_MAX_GROUPS];
    const float* d_pro_scale;   /* [Cin] or NULL */
    const float* d_pro_shift;   /* [Cin] or NULL */
    int32_t pro_relu, pro_pool;
    const float* d_epi_scale;   /* [c_off + N] or NULL */
    const float* d_epi_shift;   /* [c_off + N] or NULL */
    int32_t act;
    const void* d_R;            /* residual [M, ldr] or NULL */
    int32_t ldr;
    void* d_C;
    int32_t ldc;
    int32_t out_f32;
    /* tf.layers.dropout in training mode (modules.py:292,294), applied after the activation:
     * keep probability (0 = off) and the seed of the stateless mask (splitmix64 of the output
     * element index m*ldc + column; see drop_keep_elem in csrc/vc_gemm.hip). */
    float drop_keep;
    unsigned long long drop_seed;
    int32_t sum_groups;            /* != 0: the groups are PARTIAL SUMS of one output [M, N] (columns [0, N) of C) instead of
                                    * column blocks of it: group g convolves input channels [c_off, c_off + Cin) of X with its
                                    * own taps / pad_l / Bt, and all of them accumulate in the same tile before the epilogue
                                    * (+ residual) runs once.  This is the data gradient of conv1d_banks (the sum over the banks
                                    * of dZ_k * W_k^T, tf.gradients through modules.py:144-166) as ONE launch with the banks'
                                    * whole K.  1: one block per output tile runs every group, then the usual epilogue.
                                    * S > 1 (<= 16): the groups are dealt to S blocks per tile (g with its mirror n-1-g) and
                                    * each ADDS its bare float32 partial tile to C with atomics -- C must hold the starting
                                    * value (zeros or the residual term), no epilogue terms; for launches whose tile count
                                    * alone would leave the chip idle (summation order then varies from run to run). */
    int32_t epi_pool;              /* 1: store max(y[t], y[t+1]) inside each window of T frames (the last frame keeps
                                    * its value) = tf.layers.max_pooling1d(2, 1, 'same') of the result, fused into the
                                    * producer (modules.py:331 after :329).  Needs act = ReLU and a launch for which
                                    * vc_conv_gemm_epi_pool_supported() returns 1; vc_conv_gemm rejects it otherwise. */
    void* d_workspace;             /* optional scratch for launches that split K over workgroups (today: the 256-channel
                                    * long-K projection on the bank tiles when its row tiles alone would leave most CUs
                                    * idle): vc_conv_gemm_workspace_bytes() says how much such a launch wants (0: none).
                                    * 256-byte aligned, private to the call until it has finished on its stream (contents
                                    * need not be initialised).  NULL or too small: the unsplit form runs, same result. */
    size_t workspace_bytes;
} vc_gemm_desc;

int vc_conv_gemm(const vc_gemm_desc* desc, void* stream);
/* Bytes of d_workspace the launch described by `desc` can use (0 for nearly all launches; d_workspace itself is ignored). */
size_t vc_conv_gemm_workspace_bytes(const vc_gemm_desc* desc);
/* 1 if `desc` (with epi_pool set) can run with the pooled epilogue: the bf16 filter-bank launch that
 * maps onto the paired 256-row tiles (tiles then overlap by one frame), else 0.  Host-only. */
int vc_conv_gemm_epi_pool_supported(const vc_gemm_desc* desc);

/* Bidirectional LSTM recurrence: modules.lstm (/root/reference/modules.py:207-243 -> tf.contrib.rnn.LSTMCell with its
 * defaults: no peepholes, no projection, forget_bias 1.0, gate order i, j, f, o; bidirectional_dynamic_rnn, zero state).
 * d_xproj [n_seq*T, 8H] float32 = x W_x + b for both directions (fw | bw, 4H columns each); d_Wh_* [H, 4H] recurrent
 * halves (w_dtype); d_out [n_seq, T, 2H] (fw | bw).  H <= 512.  Reachable only with use_lstm = true, which no shipped
 * configuration sets: an any-size kernel, not a tuned one. */
int vc_lstm_bidir(const float* d_xproj, const void* d_Wh_fw, const void* d_Wh_bw, int32_t w_dtype, int32_t n_seq, int32_t T,
                  int32_t H, void* d_out, int32_t out_dtype, void* stream);

/* softmax + argmax over the last axis (encoder.py:110-111): logits float32 [M, ldl >= N] ->
 * probabilities (dtype out_dtype, row stride ldp, columns [N, ldp) zero-filled so the
 * decoder's first dense can read 16-byte rows) and int32 class ids (first maximum).  The class id lies in [0, N) for
 * every input: a row in which no logit exceeds the lowest finite float (all -inf, all -FLT_MAX, all NaN) gets class 0,
 * as tf.argmax gives on an all-equal row; NaN logits never win against a number.  The probabilities of such a row are
 * NaN (all -inf, all NaN) or 1 / N (all -FLT_MAX); every other row is unaffected.  d_class may be NULL. */
int vc_softmax_argmax(const float* d_logits, int32_t M, int32_t N, int32_t ldl,
                      void* d_prob, int32_t ldp, int32_t out_dtype, int32_t* d_class, void* stream);
/* Same, writing the probabilities twice in one launch: float32 (the API's y_pred) and a zero-padded bf16 copy (the
 * decoder's input, decoder.py:86), identical to two calls of vc_softmax_argmax. */
int vc_softmax_argmax_dual(const float* d_logits, int32_t M, int32_t N, int32_t ldl, float* d_prob, int32_t ldp,
                           void* d_prob_bf16, int32_t ldp_bf16, int32_t* d_class, void* stream);

/* Bidirectional GRU recurrence (modules.py:168-204 -> tf.nn.bidirectional_dynamic_rnn over
 * tf.contrib.rnn.GRUCell):  g = sigmoid(xg + h Wg_h);  r,u = split(g) (r first);
 * c = tanh(xc + (r*h) Wc_h);  h' = u*h + (1-u)*c, zero initial state, backward direction runs
 * t = T-1..0.  The input halves of the cell matmuls are hoisted into one GEMM beforehand:
 *   d_xproj float32 [n_seq*T, 6H] = x @ [Wg_x^fw | Wc_x^fw | Wg_x^bw | Wc_x^bw] + biases.
 *   d_Wh[dir]: recurrent weights [H, 3H] = [Wg_h | Wc_h] (rows = h index), dtype w_dtype.
 *   d_out [n_seq*T, 2H] (dtype out_dtype): fw in columns [0,H), bw in [H,2H).
 *   d_workspace: scratch of vc_gru_workspace_bytes(H, w_dtype) bytes (the register-resident
 *   kernels re-pack the weights into their per-lane order there on every call; they return VC_ERR_WORKSPACE and
 *   launch nothing when it is NULL or smaller).  1 <= H <= 1024; w_dtype and out_dtype are independent. */
size_t vc_gru_workspace_bytes(int32_t H, int32_t w_dtype);
int vc_gru_bidir(const float* d_xproj, const void* d_Wh_fw, const void* d_Wh_bw, int32_t w_dtype,
                 int32_t n_seq, int32_t T, int32_t H, void* d_out, int32_t out_dtype,
                 void* d_workspace, size_t workspace_bytes, void* stream);

/* The same recurrence on weights packed ONCE (bf16, H = 128 or 256: the two kernels that keep the weights on chip and read
 * them in a per-lane order of their own).  A model's recurrent weights do not change between inference calls, so the
 * caller packs when it loads them and again only when they change:
 *   vc_gru_form           which form a call of n_seq sequences takes.  H = 256: VC_GRU_FORM_RESIDENT (one sequence per
 *                         workgroup, 2 n_seq workgroups) when those fit ONE round of n_cu compute units, VC_GRU_FORM_MFMA (16
 *                         sequences per workgroup) beyond.  H = 128, where the two forms take the same time at 64 sequences:
 *                         resident below 32 sequences, MFMA from 32 up, whatever n_cu.  Option "gru_mfma" 0 / 1 forces
 *                         either.  n_cu <= 0: the current device's count (asked once per device).  VC_GRU_FORM_NONE for any
 *                         other H / dtype (no packed form: call vc_gru_bidir); -1 when the device cannot be asked
 *                         (vc_last_error).  Pure host code for n_cu > 0, for H = 128 and with the option set.
 *   vc_gru_packed_bytes   size of a form's image (0: no such form for H / w_dtype).
 *   vc_gru_pack           writes the image of d_Wh_fw / d_Wh_bw ([H, 3H] each, as vc_gru_bidir takes them) to d_packed
 *                         (16-byte aligned, vc_gru_packed_bytes long; VC_ERR_WORKSPACE and no launch when shorter).
 *   vc_gru_bidir_packed   vc_gru_bidir on an image; `form` must be the form the image was packed for (the two layouts
 *                         differ and carry no tag: an image of the other form gives wrong numbers, not an error).
 * Results are bit-identical to vc_gru_bidir with the same form forced. */
#define VC_GRU_FORM_NONE 0
#define VC_GRU_FORM_RESIDENT 1
#define VC_GRU_FORM_MFMA 2
int32_t vc_gru_form(int32_t H, int32_t w_dtype, int32_t n_seq, int32_t n_cu);
size_t vc_gru_packed_bytes(int32_t form, int32_t H, int32_t w_dtype);
int vc_gru_pack(int32_t form, const void* d_Wh_fw, const void* d_Wh_bw, int32_t w_dtype, int32_t H, void* d_packed,
                size_t packed_bytes, void* stream);
int vc_gru_bidir_packed(int32_t form, const float* d_xproj, const void* d_packed, size_t packed_bytes, int32_t w_dtype,
                        int32_t n_seq, int32_t T, int32_t H, void* d_out, int32_t out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training step of decoder_specs (/root/reference/decoder.py:185-263, 327-345), float32.
 * Data gradients of dense/conv layers reuse vc_conv_gemm (dX = conv of dY with the taps flipped
 * and the kernel in TF layout as the transposed operand).  The remaining pieces: */

/* Filter gradient of tf.layers.dense / conv1d, written in TF layout [taps, Cin, N]:
 *   dW[j*Cin + c, o] = sum_m X[m + j + shift0, c] * dY[m, o]    (shift0 = -pad_l; a frame of
 *   another window contributes nothing).  Operands are TRANSPOSED, frames contiguous, built by
 *   vc_transpose_pad with a zero margin of `margin` frames on both sides of every row:
 *   d_XT [Cin, ldxt], d_dYT rows [N, ldyt]; both pointers address frame 0; the allocations carry
 *   one slack row after the last (a shifted tail read may run `margin` frames past it).
 *   Groups = the banks. */
typedef struct vc_wgrad_group {
    const void* d_dYT;
    void* d_dW;
    int32_t N, taps, shift0;
    int32_t ldw;        /* row stride of d_dW (0 = N): lets a group fill a column slice */
} vc_wgrad_group;
typedef struct vc_wgrad_desc {
    const void* d_XT;
    int32_t ldxt, ldyt, Cin, M, T, margin, n_groups;
    int32_t splits_allowed;   /* != 0: every d_dW is pre-zeroed and may be accumulated with float atomics
                                 (the frame reduction is then split over more workgroups) */
    vc_wgrad_group groups[VC_GEMM_MAX_GROUPS];
} vc_wgrad_desc;
int vc_conv_wgrad(const vc_wgrad_desc* desc, void* stream);

/* XT[c, pad + m] = pro(X)[m + row_shift, c] (zero when the shifted frame leaves the window);
 * pro = optional per-channel affine, relu, time max-pool (the forward operand prologue).
 * The launch also writes the zero margins XT[c, 0 .. pad) and XT[c, pad + M .. ldt) of every row c < C and, with
 * slack_row != 0, a zero row C (d_XT then holds (C + 1) x ldt floats): the buffer need not be initialised. */
int vc_transpose_pad(const float* d_X, int32_t M, int32_t C, int32_t ld, int32_t T, const float* d_scale,
                     const float* d_shift, int32_t relu, int32_t pool, int32_t row_shift, float* d_XT,
                     int32_t ldt, int32_t pad, int32_t slack_row, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training convolutions on split-float16 operands ("f16x3"; csrc/vc_gemm16.hip).  The reference trains in float32
 * (/root/reference/decoder.py:185-263); gfx950's f32-input MFMA runs at 1/16 of the 16-bit rate.  x * s (s a power of
 * two) splits exactly into float16 hi + lo + r, |r| <= 2^-22 |x s|, and hi*hi + hi*lo + lo*hi summed in float32
 * reproduces the float32 product to 2^-22: the error of the result against float64 equals a float32 GEMM's (tests).
 * ------------------------------------------------------------------------------------------ */
/* X [M, C] float32 (row stride ldx) -> d_out16 [M, 2C] float16 = [hi plane | lo plane] of pro(X)[m] * s_w, and
 * d_row_scale[m] = 1 / s_w, s_w the power of two that puts the largest magnitude of the row's WINDOW (T rows) in
 * [2^14, 2^15) (1 for an all-zero window): the taps of a convolution stay inside a window, whose rows must share
 * their scale.  d_row_scale holds M + M / T floats: the tail is scratch.  pro = optional per-channel affine (d_scale /
 * d_shift), relu, max-pool(2, 1, same) along time inside each window -- the operand prologue of vc_conv_gemm.
 * C: a multiple of 64 up to 4096.  Two passes over X (window maxima, then the split). */
int vc_split16(const float* d_X, int32_t M, int32_t C, int32_t ldx, int32_t T, const float* d_scale, const float* d_shift,
               int32_t relu, int32_t pool, void* d_out16, float* d_row_scale, void* stream);
/* One item of vc_weights16: a TF-layout float32 kernel src [k][cin][cout] -> float16 [hi | lo] operand rows at dst.
 * mode 0 (forward operand):       row o (cout rows), column base + j * tap_stride + plane * plane_stride + c
 * mode 1 (data-gradient operand): row c (cin rows),  column base + (k - 1 - j) * tap_stride + plane * plane_stride + o
 * row_len = elements per dst row.  Items of one `group` share ONE power-of-two scale (their largest magnitude ->
 * [2^14, 2^15)); 1 / scale is written to scale_dst[0 .. scale_n) (the GEMM's per-channel d_col_scale). */
typedef struct vc_w16_item {
    const float* src;
    void* dst;
    float* scale_dst;
    int32_t k, cin, cout, mode;
    int32_t row_len, tap_stride, plane_stride, base;
    int32_t group, scale_n;
} vc_w16_item;
/* d_items: n_items items in DEVICE memory; d_gmax: n_groups uint32 of scratch.  Three launches, no host sync. */
int vc_weights16(const vc_w16_item* d_items, int32_t n_items, uint32_t* d_gmax, int32_t n_groups, void* stream);
/* C[m, c_off + n] (+)= ( sum over taps j, channels c of  X[m + j - pad_l, c] * W[n][j][c] ) * row_scale[m] * col_scale[ch]
 *                     + col_shift[ch],   X and W the float32 values vc_split16 / vc_weights16 split, SAME padding per
 * window of T rows like vc_conv_gemm.  A PAIR is two 128-column filters over the same input: widths (taps0, taps0 +
 * extra) with a common pad_l (a filter-bank pair 2p+1 / 2p+2, /root/reference/modules.py:144-166), or the two halves
 * of one 256-column filter (extra 0).  d_Bt0 / d_Bt1: [128][taps * 2C] float16, per tap [hi plane (C) | lo plane (C)].
 * ragged != 0 is the filter bank's DATA gradient (tf.gradients through modules.py:144-166): X = dZ [M, C = 128 * K],
 * bank k = 1..K contributes its 128 channels with k taps and left padding k / 2; rows of d_Bt*: [plane][bank k][tap]
 * [128] (vc_w16_item mode 1 with tap_stride 128, plane_stride 128 * K (K + 1) / 2, base 128 * k (k - 1) / 2).
 * A single-pair launch whose row tiles would not fill the chip splits K over up to 8 workgroups per row tile when
 * given vc_gemm16_workspace_bytes() of workspace (partial sums added in a fixed order: bit-identical run to run). */
typedef struct vc_gemm16_pair {
    const void* d_Bt0;
    const void* d_Bt1;
    int32_t taps0, extra, pad_l, c_off0, c_off1;
    int32_t row0;               /* first row of X the pair reads; output row r of the pair is X row row0 + r */
    int32_t nrows0, nrows1;     /* output rows each filter stores (0 = M - row0); nrows1 = -1: the pair is ONE 128-column
                                 * filter (d_Bt1 is not read and may be NULL, nothing is stored for it) */
    int32_t s_off0, s_off1;     /* atomic_splits only: first entry of d_col_scale of each filter (otherwise c_off0 / c_off1) */
} vc_gemm16_pair;
typedef struct vc_gemm16_desc {
    const void* d_X16;          /* [M, ldx >= 2C] float16 from vc_split16 */
    const float* d_row_scale;   /* [M] or NULL */
    int32_t M, T, C, ldx;
    int32_t n_pairs, ragged;
    vc_gemm16_pair pairs[16];
    const float* d_col_scale;   /* per output column, or NULL */
    const float* d_col_shift;
    float* d_C;
    int32_t ldc;
    int32_t accumulate;         /* != 0: add to the contents of d_C (after the activation: a residual) */
    int32_t act;                /* VC_ACT_NONE | VC_ACT_RELU, applied to acc * scales + shift */
    int32_t atomic_splits;      /* n >= 1: every (row tile, pair) is computed by n workgroups over n ranges of K that ADD their
                                 * partial tiles to d_C with float atomics (d_C pre-initialised; summation order not fixed).
                                 * The weight-gradient form (tf.gradients w.r.t. a conv kernel): rows = (tap, input channel) of
                                 * shifted, transposed activations from vc_transpose_split16, the contraction runs over the
                                 * frames, and a pair's c_off0 / c_off1 are ELEMENT offsets of the two filters' [rows, ldc]
                                 * gradient blocks from d_C (any alignment).  No col_shift, no ragged walk. */
    void* d_workspace;          /* 256-byte aligned, or NULL */
    size_t workspace_bytes;
} vc_gemm16_desc;
size_t vc_gemm16_workspace_bytes(int32_t M, int32_t C, int32_t n_pairs);
/* Operands of the weight-gradient form of vc_gemm16 (contraction over the frames): X [M, C] float32 (+ the prologue
 * of vc_split16) -> d_out16 rows (si * C + c), si = 0 .. n_shifts-1, each [hi plane (M) | lo plane (M)] float16 of
 * pro(X)[m + shift0 + si, c] * s_c (0 where that frame leaves its window of T), s_c the power of two that puts channel
 * c's largest magnitude in [2^14, 2^15); d_row_scale[si * C + c] = 1 / s_c.  d_row_scale holds (n_shifts + 1) * C
 * floats (the tail is scratch).  M and C: multiples of 64. */
int vc_transpose_split16(const float* d_X, int32_t M, int32_t C, int32_t ldx, int32_t T, const float* d_scale,
                         const float* d_shift, int32_t relu, int32_t pool, int32_t shift0, int32_t n_shifts, void* d_out16,
                         float* d_row_scale, void* stream);
int vc_gemm16(const vc_gemm16_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * MX-FP8 inference of the decoder's filter banks and the projection behind them (csrc/vc_mx8.hip; opt-in through
 * VariableStore(compute_dtype='mxfp8')).  Format: OCP MX-FP8, e4m3fn elements, one E8M0 scale byte 2^(code - 127) per
 * 32 consecutive K elements of a row.  Scale rule: the smallest e with amax <= 448 * 2^e (clamped to [-127, 127]),
 * elements RNE(x * 2^-e) with subnormals kept, nothing saturates; an all-zero block has scale code 0 and 0x00
 * elements (csrc/vc_mx8.h holds the one device definition, tests/mx8_ref.py the CPU reference).
 * ------------------------------------------------------------------------------------------ */
/* X [M, C] bf16 (x_dtype VC_BF16) or float32 (VC_F32), row stride ldx elements -> d_Q [M, C] e4m3fn codes and d_S
 * [M, C / 32] E8M0 scales, both dense.  C: a multiple of 32.  Used for the filter-bank input
 * (the reference's modules.py:160, the bank's tf.layers.conv1d input) and for packing the weights, transposed to
 * [Cout, taps * Cin] the way vc_conv_gemm stores them (blocks = (output channel, tap, 32 input channels)). */
int vc_mx8_quantize(const void* d_X, int32_t x_dtype, int32_t M, int32_t C, int32_t ldx, void* d_Q, void* d_S, void* stream);
#define VC_MX8_MAX_GROUPS 32
#define VC_MX8_OUT_MX 0         /* out_mode: MX-FP8 codes d_C [M, n_out] + scales d_Cs [M, n_out / 32] */
#define VC_MX8_OUT_BF16 1       /* bf16 d_C [M, n_out] */
#define VC_MX8_OUT_F32 2        /* float32 d_C [M, n_out] (the epilogue's values before any quantisation: tests) */
/* One 128-channel filter of a launch: d_W [128][taps * Cin] e4m3fn and d_Ws [128][taps * Cin / 32] from
 * vc_mx8_quantize, output channels [c_off, c_off + 128), SAME left padding pad_l. */
typedef struct vc_mx8_group {
    const void* d_W;
    const void* d_Ws;
    int32_t taps, pad_l, c_off, reserved;
} vc_mx8_group;
/* Y[m, c_off + n] = epi( sum over taps j, channels c of X[m + j - pad_l, c] * W[n][j][c] ), X and W the dequantised MX
 * operands, SAME zero padding inside each window of T rows, float32 accumulation.  Groups are taken two at a time
 * (2g, 2g + 1) by one workgroup over 128 frames, so they must come in pairs that share pad_l -- filter-bank widths
 * (2p+1, 2p+2) -- or be the halves of one 256-channel filter; a single group (128 outputs) is allowed.
 * epi = d_epi_scale[ch] * acc + d_epi_shift[ch] (folded inference BatchNorm), then relu (act = VC_ACT_RELU), then with
 * pool != 0 max_pooling1d(2, 1, 'same') along time inside each window (the reference's modules.py:331), then the
 * output conversion of out_mode.  Shapes: Cin a multiple of 64, n_out a multiple of 32, taps 1..32.
 * Replaces: conv1d_banks + max_pooling1d (the reference's modules.py:144-166, 331) as ONE launch writing MX-FP8, and
 * conv1d_1 (the reference's modules.py:333-335) reading it and writing bf16.  A launch without pool and with at most
 * two groups splits K over workgroups when given vc_mx8_conv_workspace_bytes() of workspace (float32 partial sums,
 * reduced in a fixed order by a second launch: bit-identical run to run; out_mode BF16 / F32 only). */
typedef struct vc_mx8_conv_desc {
    const void* d_X;            /* [M, Cin] e4m3fn codes */
    const void* d_Xs;           /* [M, Cin / 32] E8M0 */
    int32_t M, T, Cin, n_groups;
    vc_mx8_group groups[VC_MX8_MAX_GROUPS];
    const float* d_epi_scale;   /* [n_out] */
    const float* d_epi_shift;   /* [n_out] */
    int32_t act, pool, out_mode, n_out;
    void* d_C;
    void* d_Cs;                 /* VC_MX8_OUT_MX only */
    void* d_workspace;          /* 256-byte aligned, or NULL (no split) */
    size_t workspace_bytes;
} vc_mx8_conv_desc;
size_t vc_mx8_conv_workspace_bytes(const vc_mx8_conv_desc* desc);
int vc_mx8_conv(const vc_mx8_conv_desc* desc, void* stream);

/* Train-mode FusedBatchNorm bookkeeping (modules.py:77-84, is_training): batch mean / biased
 * variance of X [M, C] -> scale/shift (consumed by the next launch's prologue or vc_affine_act),
 * saved mean/rstd for backward, moving statistics updated in place (decay, Bessel-corrected
 * variance).  d_workspace: vc_stats_workspace_floats(M, C) floats. */
size_t vc_stats_workspace_floats(int32_t M, int32_t C);
int vc_bn_train_stats(const float* d_X, int32_t M, int32_t C, int32_t ld, const float* d_gamma,
                      const float* d_beta, float* d_moving_mean, float* d_moving_var, float decay, float eps,
                      float* d_scale, float* d_shift, float* d_mean, float* d_rstd, float* d_workspace,
                      void* stream);
/* out = act(X * scale[c] + shift[c]) + R   (any of scale/shift/R may be NULL). */
int vc_affine_act(const float* d_X, const float* d_scale, const float* d_shift, int32_t relu, const float* d_R,
                  float* d_out, size_t n, int32_t C, void* stream);
/* BatchNorm backward fused with what follows the norm: mode 0 none, 1 relu, 2 relu + time
 * max-pool (modules.py:165,331: d_G is the gradient w.r.t. the pooled tensor).  Writes dX (raw
 * conv output gradient), dgamma, dbeta. */
int vc_bn_backward(const float* d_G, const float* d_X, int32_t M, int32_t C, int32_t ld, int32_t T,
                   const float* d_gamma, const float* d_scale, const float* d_shift, const float* d_mean,
                   const float* d_rstd, int32_t mode, float* d_dX, float* d_dgamma, float* d_dbeta,
                   float* d_workspace, void* stream);
/* The relu / max-pool routing vc_bn_backward(mode 2) applies (modules.py:165 relu, :331 max_pooling1d(2, 1, same)), one
 * byte per element of X [M, C] (output contiguous, row stride C): bit 0: bn(X) > 0; bit 1: the element receives the
 * gradient of its own frame's pool output (last frame of a window, or >= its successor); bit 2: it receives the
 * previous frame's (strictly greater than its predecessor).  Same device function as the backward pass itself; where
 * two float32 pre-activations tie to within rounding TensorFlow's float32 kernels would be equally arbitrary, so a
 * float64 restatement has to be handed these decisions to be comparable element by element (tests). */
int vc_bn_post_routing(const float* d_X, int32_t M, int32_t C, int32_t ld, int32_t T, const float* d_scale,
                       const float* d_shift, uint8_t* d_bits, void* stream);
/* dZ = (Y > 0) ? dY * inv_keep : 0 for Y = dropout(relu(Z)) (modules.py:291-294). */
int vc_relu_dropout_backward(const float* d_dY, const float* d_Y, float inv_keep, float* d_dZ, size_t n, void* stream);
/* highwaynet backward gate arithmetic (modules.py:315-318) on re-computed pre-activations in the
 * forward's paired column layout [M, NP]; writes d(pre) [M, NP] and the direct path dO*(1-T). */
int vc_highway_backward(const float* d_pre, int32_t NP, const float* d_X, const float* d_dO, int32_t M, int32_t H,
                        float* d_dpre, float* d_dXd, void* stream);
/* out[c] (+)= sum_m X[m, c]  (bias gradients); d_workspace: 64 * C floats. */
int vc_col_sum(const float* d_X, int32_t M, int32_t C, int32_t ld, float* d_out, int32_t accumulate,
               float* d_workspace, void* stream);
int vc_fill(float* d_p, float value, size_t n, void* stream);
/* out[m][c] = a * X[m][c] + b * Y[m][c] over [M, C] float32 views with row strides ldx / ldy / ldo (out may alias X or
 * Y).  decoder_specs._build_model's teacher-forced stage-2 input, /root/reference/decoder.py:148-152:
 * inputs_step2 = f_mel_pred * y_mel + (1 - f_mel_pred) * target_mel, and its gradient dY_mel += f_mel_pred * dX. */
/* Kernel-layout copies of many convolution weights in ONE launch (training: after every optimiser step).
 * d_items: DEVICE array of n_items descriptors; src = TF-layout kernel [k, cin, cout] float32 (tf.layers.conv1d /
 * dense with k = 1: /root/reference/modules.py:104-140), dst float32:
 *   mode 0: [cout, k*cin]  = the transposed operand vc_conv_gemm's groups take (vc_gemm_group.d_Bt),
 *   mode 1: [cin, k*cout] with the taps reversed = the operand of the data-gradient convolution (decoder.py:236-246's
 *           tf.gradients through conv1d). */
typedef struct vc_layout_item {
    const float* src;
    float* dst;
    int32_t k, cin, cout, mode;
} vc_layout_item;
int vc_weight_layouts(const vc_layout_item* d_items, int32_t n_items, void* stream);
int vc_axpby(const float* d_X, int32_t ldx, float a, const float* d_Y, int32_t ldy, float b, float* d_out, int32_t ldo,
             int32_t M, int32_t C, void* stream);
/* loss = weight * mean((y - t)^2) (decoder.py:187-189); optional d_dY = 2*weight/n * (y - t).
 * y/t are contiguous [n/C, C]; d_dY is written with row stride ld_dy >= C (padding columns are
 * left untouched).  d_workspace: 256 floats; d_loss: 1 float on the device (no host sync). */
int vc_mse_loss(const float* d_y, const float* d_t, size_t n, float weight, float* d_dY, int32_t C, int32_t ld_dy,
                float* d_loss, float* d_workspace, void* stream);
/* LSTM recurrence in training mode (use_lstm; /root/reference/modules.py:207-243: tf.contrib.rnn.LSTMCell, forget_bias 1.0,
 * under bidirectional_dynamic_rnn): d_xproj [n_seq*T, 8H] = per direction the input projections (i | j | f | o) incl. bias,
 * d_Wh_* [H, 4H] the recurrent rows of the cell kernel; stores the hidden states d_out [n_seq*T, 2H], the ACTIVATED gates
 * d_gates [2][n_seq*T, 4H] and the cell states d_cstate [2][n_seq*T, H].  float32, H <= 512.  (No shipped configuration
 * enables use_lstm: any-size kernels, not tuned ones.) */
int vc_lstm_train_forward(const float* d_xproj, const float* d_Wh_fw, const float* d_Wh_bw, int32_t n_seq, int32_t T,
                          int32_t H, float* d_out, float* d_gates, float* d_cstate, void* stream);
/* BPTT of the above: d_dout [n_seq*T, 2H] -> d_dpre [n_seq*T, 8H], the gradient w.r.t. the gate pre-activations in the
 * layout of d_xproj.  d_WhT_* [4H, H]: the recurrent weights transposed. */
int vc_lstm_backward(const float* d_dout, const float* d_gates, const float* d_cstate, const float* d_WhT_fw,
                     const float* d_WhT_bw, int32_t n_seq, int32_t T, int32_t H, float* d_dpre, void* stream);
/* Encoder loss and metrics (/root/reference/encoder.py:134-150): out3 = [mean softmax cross-entropy
 * with float labels, accuracy of argmax(logits) vs argmax(target), mean squared error of the
 * posteriors]; optional d_dlogits [M, ldd] = (softmax * sum(target) - target) / M.
 * d_workspace: 3 * M floats; results stay on the device. */
int vc_softmax_ce(const float* d_logits, const float* d_target, int32_t M, int32_t C, int32_t ldl, float* d_dlogits,
                  int32_t ldd, float* d_out3, float* d_workspace, void* stream);
/* tf.train.AdamOptimizer update on flat buffers (decoder.py:236-246): g is first multiplied by
 * grad_scale (1/world for data-parallel averaging), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) from the host,
 * p -= lr_t * m / (sqrt(v) + epsilon). */
int vc_adam_step(float* d_param, const float* d_grad, float* d_m, float* d_v, size_t n, float lr_t, float beta1,
                 float beta2, float epsilon, float grad_scale, void* stream);
/* GRU recurrence in training mode: like vc_gru_bidir (float32 weights) but also stores the gate
 * activations d_gates [2][n_seq*T, 3H] (r | u | c) and r*h d_rh [2][n_seq*T, H]. */
int vc_gru_train_forward(const float* d_xproj, const float* d_Wh_fw, const float* d_Wh_bw, int32_t n_seq,
                         int32_t T, int32_t H, float* d_out, float* d_gates, float* d_rh, void* stream);
/* BPTT of the above: d_dout [n_seq*T, 2H] -> d_dpre [n_seq*T, 6H] = gradient w.r.t. the gate
 * pre-activations in the layout of d_xproj (input/recurrent weight gradients follow as GEMMs).
 * d_WhT_* [3H, H]: optional transposed copies of the recurrent weights; with them several windows
 * share a workgroup and the W^T matvecs read coalesced rows. */
int vc_gru_backward(const float* d_dout, const float* d_out, const float* d_gates, const float* d_Wh_fw,
                    const float* d_Wh_bw, const float* d_WhT_fw, const float* d_WhT_bw, int32_t n_seq,
                    int32_t T, int32_t H, float* d_dpre, void* stream);

/* ---- Griffin-Lim vocoder ---------------------------------------
 * Replaces audio_lib.griffin_lim_alg / from_power_to_wav / calc_inv_preemphasis
 * (/root/reference/audio_lib.py:249-274, 278-308, 31-47; called from test.py:146-168, 253-275,
 * 346-362).  Spectrogram layout is frame-major: [batch, max_frames, 1 + n_fft/2] (the decoder's
 * y_stft layout, i.e. the TRANSPOSE of the [bins, frames] array librosa works on). */
typedef struct vc_vocoder_plan vc_vocoder_plan;

/* Device tables (padded window, DFT twiddles).  n_fft <= 0 => n_fft = win_length
 * (audio_lib.py:251-252).  h_window: host float64[win_length] or NULL for periodic hann (librosa's
 * default, the only window the reference uses here).  n_fft == 400 takes the 25 x 16 split
 * transform; other (even) sizes take a direct DFT. */
int vc_vocoder_plan_create(int32_t win_length, int32_t hop_length, int32_t n_fft, const double* h_window,
                           vc_vocoder_plan** out_plan);
void vc_vocoder_plan_destroy(vc_vocoder_plan* plan);
/* Samples librosa.istft returns for n_frames frames: hop_length * (n_frames - 1). */
int32_t vc_vocoder_num_samples(const vc_vocoder_plan* plan, int32_t n_frames);
/* The caller-owned workspace of vc_griffin_lim_f32 / vc_griffin_lim_momentum_f32 (host arithmetic only; 0 for a NULL plan,
 * batch <= 0 or max_frames <= 0; too small: VC_ERR_INVALID before any launch).  With align256(x) = x rounded up to 256,
 * N = n_fft and FB = align256(batch * max_frames * N * 4), in this order:
 *     offset 0             frame buffer 0   [batch, max_frames, N] float32   the windowed synthesis frames w[n] * irfft(S_f)[n]
 *     offset FB            frame buffer 1   the same
 *     with trace != 0      two waveforms [batch, hop * (max_frames - 1)] float32 (row stride hop * (max_frames - 1)), each
 *                          align256(batch * hop * (max_frames - 1) * 4) bytes: waveform i of a traced run goes to number i & 1
 *     momentum only        the state R_{i-1}, align256(batch * max_frames * slots * 8) bytes, one float2 (re, im) per slot:
 *                          [batch, max_frames, 13, 16] on the 400-point path, where slot (k1, k2) holds bin k1 + 25 k2 of the
 *                          400-point spectrum of the frame (k1 < 13 and k2 < 16 give 208 distinct bins up to 387; a bin above
 *                          200 is stored as computed, the conjugate of bin 400 - k to rounding);
 *                          [batch, max_frames, 1 + N/2] otherwise
 *     256 spare bytes
 *     vc_vocoder_workspace_bytes          = 2 FB + (trace ? 2 align256(batch * hop * (max_frames - 1) * 4) : 0) + 256
 *     vc_vocoder_workspace_bytes_momentum = the same + align256(batch * max_frames * slots * 8)
 * Launch i (0-based; launch 0 reads no frames) reads frame buffer i & 1 and writes the other, so after num_iters launches the final frames (those d_wav
 * is the overlap-add of) are in frame buffer num_iters & 1 and the frames the last launch read in the other.  With momentum
 * > 0 and num_iters >= 2 the state holds R_{num_iters-1}, the analysis of the last launch before its projection.  Rows at or
 * beyond n_frames[b] of the frame buffers and of the state are never written; nothing is read before it is written. */
size_t vc_vocoder_workspace_bytes(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames, int32_t trace);

/* audio_lib.py:289-298: P = max(0, P); optional P = (mean(P)/mean(P**realse)) * P**realse (means
 * over the utterance); amp = sqrt(db_to_power(P / P_dB_norm_factor - 80)).  d_P, d_amp
 * [batch, max_frames, n_bins]; rows >= n_frames[b] are written as 0.  d_n_frames may be NULL. */
int vc_power_to_amp(const float* d_P, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_bins,
                    float P_dB_norm_factor, float realse, float* d_amp, void* stream);

/* audio_lib.py:249-274.  d_amp, d_phase0 [batch, max_frames, 1+n_fft/2] (phase0 in radians: the
 * reference draws pi * U[0,1) on the host, audio_lib.py:255 -- the caller supplies it so a seeded
 * run is reproducible); d_n_frames int32 [batch] or NULL (all max_frames); each utterance needs
 * hop*(n_frames-1) > n_fft/2.  d_wav [batch, wav_stride] receives hop*(n_frames[b]-1) samples per
 * utterance, zero beyond.  d_trace: NULL, or float32 [num_iters, batch] that receives
 * sum_n (wav_i[n] - wav_{i-1}[n])^2 for i >= 1 (the reference's verbose print is
 * sqrt(that / n_samples)); costs one extra launch per iteration.
 * num_iters launches of the fused projection kernel + 1 overlap-add on `stream`. */
int vc_griffin_lim_f32(const vc_vocoder_plan* plan, const float* d_amp, const float* d_phase0,
                       const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t num_iters,
                       float* d_wav, int32_t wav_stride, float* d_trace, void* d_workspace, size_t workspace_bytes,
                       void* stream);

/* Fast Griffin-Lim (Perraudin, Balazs & Sondergaard 2013), librosa's / torchaudio's formulation, with the
 * state and iteration count of audio_lib.py:249-274 (num_iters ISTFTs, num_iters - 1 projections).  With
 * beta = momentum / (1 + momentum) and R_0 = 0, for i = 1 .. num_iters - 1:
 *     R_i = STFT(ISTFT(S_{i-1}))        (complex)
 *     C_i = R_i - beta * R_{i-1}
 *     S_i = amp * C_i / |C_i|           (a zero C_i gets phase 0)
 * and wav = ISTFT(S_{num_iters-1}).  momentum must be finite and in [0, 1), else VC_ERR_INVALID before any
 * launch.  momentum == 0 launches exactly what vc_griffin_lim_f32 launches (bit-identical, and needs only
 * vc_vocoder_workspace_bytes); with num_iters <= 2 the momentum never acts and the result is bit-identical
 * to momentum 0.  momentum > 0 needs vc_vocoder_workspace_bytes_momentum bytes, 16-byte aligned: R_{i-1}
 * per frame, 13 x 16 float2 (1,664 bytes) on the 400-point path, 1 + n_fft/2 float2 on the generic one,
 * read and rewritten once per iteration.  Other arguments, the trace and the launch count as
 * vc_griffin_lim_f32; hipGraph-capturable like every launch call here. */
size_t vc_vocoder_workspace_bytes_momentum(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames,
                                           int32_t trace);
int vc_griffin_lim_momentum_f32(const vc_vocoder_plan* plan, const float* d_amp, const float* d_phase0,
                                const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t num_iters,
                                float momentum, float* d_wav, int32_t wav_stride, float* d_trace, void* d_workspace,
                                size_t workspace_bytes, void* stream);

/* audio_lib.py:301-306 in place on d_wav [batch, wav_stride] (first hop*(n_frames[b]-1) samples):
 * y[n] = x[n] + coeff*y[n-1] (skipped when coeff == 0), then y *= mean_abs_amp_norm / mean|y|
 * (skipped when mean_abs_amp_norm <= 0). */
int vc_inv_preemphasis_normalize(const vc_vocoder_plan* plan, float* d_wav, const int32_t* d_n_frames, int32_t batch,
                                 int32_t max_frames, int32_t wav_stride, float coeff, float mean_abs_amp_norm,
                                 void* stream);

/* ---- highway chain (modules.py:297-319 applied L times, modules.py:342-345) ------------------
 * All L highwaynet layers of a CBHG block in one launch (bf16, H = 128 or 256): a block keeps its
 * 128 frames in LDS across the layers, weights stream from L2 in MFMA fragment order; optionally
 * followed, on the same on-chip activations, by the GRU's input projection (modules.py:346,
 * GRUCell x-halves of both directions: a dense layer H -> n_proj with float32 output).
 * vc_highway_pack: d_Bt [n_cols, H] bf16, K contiguous (for the highway layers the paired [2H, H]
 * matrix of vc_conv_gemm's VC_GEMM_HIGHWAY mode: rows 64q..64q+31 = dense1 columns of units 32q..,
 * rows 64q+32.. = dense2) -> d_packed [n_cols*H] bf16 in fragment order.
 * vc_highway_chain: d_packed / d_bias are HOST arrays of n_layers (0..8) device pointers (bias:
 * float32 [2H], paired order).  d_Y [M, ldy] bf16 receives the last layer's output (NULL: not
 * stored; may equal d_X).  d_proj_packed (NULL: no tail) / d_proj_bias [n_proj] / d_P [M, ldp]
 * float32; any n_proj that is a multiple of 64 is served, also one below the 64 columns per wave of a pass (a wave without
 * a column group loads nothing).  Bit-identical to n_layers launches of vc_conv_gemm(VC_GEMM_HIGHWAY) + one dense launch. */
int vc_highway_pack(const void* d_Bt, int32_t n_cols, int32_t H, void* d_packed, void* stream);
int vc_highway_chain(const void* d_X, int32_t M, int32_t H, int32_t ldx, int32_t n_layers,
                     const void* const* d_packed, const float* const* d_bias, void* d_Y, int32_t ldy,
                     const void* d_proj_packed, const float* d_proj_bias, int32_t n_proj, float* d_P, int32_t ldp,
                     void* stream);

/* ---- the encoder's pre-recurrence chain in one launch -------------------------------------------
 * encoder.py:101-107 up to the GRU: prenet (modules.py:274-295) -> conv1d_banks + bn + relu
 * (modules.py:144-166) -> max_pooling1d (modules.py:331) -> conv1d k=3 + bn + relu -> conv1d k=3 + bn
 * + residual (modules.py:334-340) -> highwaynet x n_highway (modules.py:342-345) -> the x-halves of
 * the bidirectional GRU's cell matmuls (modules.py:346, 168-204), for the SHIPPED encoder shape
 * (hp/encoder_cfg_d.json: 80 features, prenet 80 -> 40, 6 banks x 128 filters, GRU of 40 units; bf16
 * weights, inference).  vc_cbhg_front_supported() says whether a shape takes this path; callers run
 * the per-layer entry points (vc_conv_gemm, vc_highway_chain) otherwise -- same results within bf16
 * rounding (different float32 summation order).  The pool between the banks and conv1d_1 orders either zero
 * below every positive value (the signed integer maximum of the post-ReLU values, as vc_conv_gemm's pro_pool = 2).
 *
 * Weights are handed over in MFMA fragment order, built with vc_mfma_pack from row-major bf16
 * matrices W [rows, K] (row = output channel, K contiguous):
 *   packed[(tile * nks + s) * 64 + lane][e] = W[32 tile + (lane & 31)][kmap(16 s + 8 (lane >> 5) + e)],
 *   tile < ceil(rows / 32), s < nks = ceil(K / 16), zero outside W;
 *   kmap = identity (chained = 0) or, for a layer that consumes the previous layer's result tile
 *   straight from registers (chained = 1), kmap(16 s + 8 h + e) = 32 (s>>1) + 8 (2 (s&1) + (e>>2)) + 4 h + (e&3).
 * Matrices (TF kernels transposed to [out, in]):
 *   d_pk_dense1  [80, 80] plain;  d_pk_dense2 [40, 80] chained;
 *   d_pk_bank    the 6 filters [128, 40 k] (K index = tap * 40 + channel), plain, concatenated k = 1..6;
 *   d_pk_proj1   [40, 2304] with K re-ordered to (width k-1, 32-channel slice w, tap, 16-channel half s, 16):
 *                column ((((k-1) * 4 + w) * 3 + tap) * 2 + s) * 16 + j  <-  conv1d_1 kernel[tap, (k-1) * 128 + 32 w + 16 s + j, :], plain;
 *   d_pk_proj2   [40, 120] (K index = tap * 40 + channel), plain;
 *   d_pk_highway[l] the paired [128, 40] matrix (rows 64 q .. +31 dense1 of units 32 q .., rows 64 q + 32 .. dense2), chained;
 *   d_pk_gru     [240, 40] (rows: fw gates 80 | fw candidate 40 | bw gates 80 | bw candidate 40), chained.
 * d_coef: ONE float32 array of vc_cbhg_front_coef_floats() (= 3232) values, every vector zero padded to its slot:
 *   [0, 96) dense1 bias | [96, 160) dense2 bias | [160, 1184) bank scale | [1184, 2208) bank shift (folded batch
 *   norm of the 768 bank channels) | [2208, 2272) conv1d_1 scale | [2272, 2336) shift | [2336, 2400) conv1d_2 scale |
 *   [2400, 2464) shift | [2464, 2720) GRU bias (240) | [2720 + 128 l, +128) highway layer l biases, paired order.
 * d_x [n_windows * T, ldx] float32 (x_f32 = 1) or bf16; d_xproj [n_windows * T, ldp] float32 receives
 * columns [0, 240).  A window whose features are NaN comes out as NaN (the ReLUs of this launch keep a NaN) and does not
 * reach its neighbours. */
#define VC_CBHG_FRONT_MAX_HIGHWAY 4
typedef struct vc_cbhg_front_desc {
    const void* d_x;
    int32_t x_f32, ldx;
    int32_t n_windows, T;
    int32_t n_features, prenet_units, width, n_banks, bank_filters, n_highway, gru_units;
    const void *d_pk_dense1, *d_pk_dense2, *d_pk_bank, *d_pk_proj1, *d_pk_proj2, *d_pk_gru;
    const void* d_pk_highway[VC_CBHG_FRONT_MAX_HIGHWAY];
    const float* d_coef;
    float* d_xproj;
    int32_t ldp;
} vc_cbhg_front_desc;
int vc_mfma_pack(const void* d_W, int32_t rows, int32_t K, int32_t ldw, int32_t chained, void* d_packed, void* stream);
int32_t vc_cbhg_front_coef_floats(void);
int vc_cbhg_front_supported(int32_t n_features, int32_t prenet_units, int32_t width, int32_t n_banks,
                            int32_t bank_filters, int32_t n_highway, int32_t gru_units, int32_t T);
int vc_cbhg_front(const vc_cbhg_front_desc* desc, void* stream);

/* ---- prenet as one launch (modules.py:274-295, inference) ----------------------------------------
 * Y = relu(relu(X W1 + b1) W2 + b2) in bf16 for the decoder stages' shapes (cin_padded -> units1 -> units2 =
 * 64 -> 256 -> 128 and 80 -> 512 -> 256; vc_prenet_chain_supported() tells, other shapes take two vc_conv_gemm
 * launches): the intermediate stays in registers.  d_pk1 = vc_mfma_pack(W1^T [units1, cin_padded], chained = 0),
 * d_pk2 = vc_mfma_pack(W2^T [units2, units1], chained = 1); d_b1 [units1], d_b2 [units2] float32;
 * d_X [M, ldx] bf16, or float32 with x_f32 = 1 (converted on load: y_mel of the previous stage), padding columns zero; d_Y [M, ldy] bf16.  Same bf16 rounding points as the two launches,
 * float32 sums in the same K order: bit-identical to the two launches on the device (tests/test_chain_kernels_gpu.py asserts
 * equality at M = 1 .. 257 for both shapes and both kernel forms). */
int vc_prenet_chain_supported(int32_t cin_padded, int32_t units1, int32_t units2);
int vc_prenet_chain(const void* d_X, int32_t x_f32, int32_t M, int32_t ldx, int32_t cin_padded, int32_t units1, int32_t units2,
                    const void* d_pk1, const float* d_b1, const void* d_pk2, const float* d_b2, void* d_Y, int32_t ldy,
                    void* stream);

/* ---- on-device feature cache -----------------------------------
 * dst[r, :] = src[index[r], :] for index[r] >= 0, else pad_row (zeros when d_pad_row is NULL).
 * Rows are row_bytes wide (multiple of 4).  Replaces the h5py slicing + np.array stacking of
 * sound_ds.py:262-350, ARCTIC_reader.py:277-362, TIMIT_reader.py:474-523 (and packs front-end
 * output into the ragged cache, ARCTIC_reader.py:109-175 / TIMIT_reader.py:144-210). */
int vc_gather_rows(const void* d_src, const int64_t* d_index, const void* d_pad_row, int64_t n_rows,
                   int32_t row_bytes, void* d_dst, void* stream);

/* float32 <-> bf16 conversion of a contiguous buffer (weights preparation, I/O). */
int vc_convert(const void* d_src, int32_t src_dtype, void* d_dst, int32_t dst_dtype, size_t n, void* stream);

/* ---- device-resident batched conversion (conversion.convert_batch; test.py:46-138 without the host) -----------
 * Three streaming launches between the front-end, the decoder and the vocoder.  Each validates on the host, allocates
 * nothing, writes every destination element exactly once (no memset, no atomics) and is hipGraph-capturable.  Their
 * tables live on the device and are read by the kernel: an entry that points outside the source yields zero rows,
 * never a read outside it.  16-byte stores whenever a destination slab (T * C, out_frames * C, max_frames * n_bins
 * floats) is a multiple of 4 floats; 16-byte loads when, in addition, C % 4 == 0 (80, 64); rows of 201 or 61 values
 * are read element by element (their rows do not start on 16-byte boundaries).
 *
 * vc_cut_windows: d_dst [n_windows, T, C] <- d_src [batch, max_frames, C] float32.  d_win_tab int32 [n_windows][2] =
 * (utterance, first frame): window w, row t is row first_frame + t of that utterance, or zeros where
 * first_frame + t >= min(n_frames[utterance], max_frames) -- the reference's zero padding of the features to a
 * multiple of T (test.py:92-101) without a padded copy.  d_n_frames int32 [batch], NULL = max_frames everywhere.  One
 * launch cuts pass 0 and the half-shifted pass 1 of every utterance.  (vc_gather_rows computes the same function from
 * one int64 per ROW: 8 * n_windows * T bytes of index to build and upload per call, 256 KB for 16 utterances of 5 s,
 * against 8 bytes per WINDOW here, 640 bytes; it also moves 4 bytes per lane.  Hence this export.) */
int vc_cut_windows(const float* d_src, const int32_t* d_win_tab, const int32_t* d_n_frames, int32_t batch,
                   int32_t max_frames, int32_t n_windows, int32_t T, int32_t C, float* d_dst, void* stream);

/* vc_compound_stitch: d_dst [batch, out_frames, C] float32 <- d_src [n_windows, T, C] (src_dtype VC_F32 or VC_BF16,
 * bf16 widened exactly), T a multiple of 4.  d_utt_tab int32 [batch][3] = (first pass-0 window w0, first pass-1
 * window w1 or -1, N): the utterance owns pass-0 windows w0 .. w0+N-1 and pass-1 windows w1 .. w1+N-2.  With q = T/4,
 * h = T/2, output row t of utterance b is
 *     t >= N*T                  zeros
 *     N == 1 or w1 < 0          pass 0, window t / T, frame t % T (the plain reshape, test.py:134-138)
 *     t < T-q                   pass 0, window 0, frame t
 *     t >= N*T - (T-q)          pass 0, window N-1, frame t - (N-1)*T
 *     otherwise                 j = (t-(T-q)) / h, r = (t-(T-q)) % h: even j -> pass 1, window j/2, frame q+r;
 *                               odd j -> pass 0, window (j+1)/2, frame q+r
 * which is `compound` (test.py:46-84).  Pure data movement: bit-exact.  d_amp (NULL, or float32 like d_dst; source
 * must be VC_F32): the fused flavour for the power spectrum also writes the vocoder's magnitude,
 * amp = exp10(0.05 * (max(0, P) / P_dB_norm_factor - 80)) in the rows t < N*T and 0 beyond -- what vc_power_to_amp
 * writes for realse == 1 and n_frames = N*T, bit for bit, in one pass over the data instead of three.  For
 * realse != 1 the two means over the utterance are needed first: the caller passes d_amp = NULL and runs the
 * stitched spectrum through vc_power_to_amp (the existing launch is reused; no reduction pre-pass here).
 * Grid: (tiles of 1,024 values, utterance). */
int vc_compound_stitch(const void* d_src, int32_t src_dtype, const int32_t* d_utt_tab, int32_t batch, int32_t n_windows,
                       int32_t T, int32_t C, int32_t out_frames, float* d_dst, float* d_amp, float P_dB_norm_factor,
                       void* stream);

/* vc_phase_init: Griffin-Lim's initial phase (audio_lib.py:255: pi * U[0, 1)) drawn on the device.
 * d_phase [batch, max_frames, n_bins] float32: phase[b, f, k] = float32(pi) * u for f < n_frames[b], 0 beyond, with
 * u = (x >> 8) * 2^-24 (exact in float32, so the value is one correctly rounded product) and x a word of
 * Philox4x32-10 (Salmon, Moraes, Dror & Shaw, SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85): with e = f * n_bins + k, counter = (e / 4, utt_id[b], 0, 0), key = (low, high 32 bits of seed; any 64-bit pattern),
 * x = output word e % 4.  An utterance's phase therefore depends on (seed, utt_id, f, k) alone: not on its place in
 * the batch, on max_frames or on the other utterances.  d_utt_id int32 [batch], NULL = 0 .. batch-1; d_n_frames int32
 * [batch], NULL = max_frames.  max_frames * n_bins < 2^34. */
int vc_phase_init(const int32_t* d_n_frames, const int32_t* d_utt_id, int32_t batch, int32_t max_frames, int32_t n_bins,
                  int64_t seed, float* d_phase, void* stream);

/* vc_phase_spsi: a deterministic initial phase for Griffin-Lim computed from the magnitudes alone -- single-pass
 * spectrogram inversion (Beauregard, Harish & Wyse 2015): pick every frame's spectral peaks, interpolate each peak's
 * frequency, advance its phase by hop * frequency, lock the neighbouring bins to their peak.  No seed, no utterance id,
 * no generator state: an utterance's phase does not depend on its place in the batch, on max_frames or on the other
 * utterances.  Added without a version bump (a new export; no existing signature moved).
 *
 * d_amp [batch, max_frames, n_bins] float32, frame-major (the layout vc_griffin_lim_f32 takes), n_bins = 1 + n_fft/2;
 * d_n_frames int32 [batch], NULL = max_frames; d_phase like d_amp.  The definition is exact: phase is kept as an unsigned
 * 32-bit fraction of a turn (addition wraps mod 2^32 = one turn), and per frame t, from m = amp[u, t, :] only:
 *   peak   bin k in 1 .. n_bins-2 with m[k] > m[k-1] and m[k] > m[k+1] (strict float32 comparisons);
 *   owner  a peak owns itself; a non-peak bin b in 1 .. n_bins-2 is owned by the peak k > b if m[j] < m[j+1] for all
 *          b <= j < k, by the peak k < b if m[j] < m[j-1] for all k < j <= b, and by the higher-frequency one if both
 *          hold (a valley); bins 0 and n_bins-1 and every bin no peak reaches (plateaus, all-equal frames, monotone
 *          ramps) are unowned;
 *   inc(k) = uint32((uint64((hop*k) % n_fft) << 32) / n_fft) + uint32(llrint((double)p * ((double)hop * 2^32 / n_fft))),
 *          p = 0.5f * (a - d) / ((a - 2.0f*c) + d) in float32 (this association, IEEE division) with
 *          (a, c, d) = m[k-1], m[k], m[k+1];
 *   v(t, b) = v(t-1, k) + inc(k) + (((b - k) & 1) << 31) if b is owned by k, v(t-1, b) otherwise, v(-1, .) = 0 -- the
 *          half turn on every odd neighbour is the phase slope of a window centred at n_fft/2 in a frame that starts at
 *          sample 0, which is what the vocoder's STFT uses;
 *   phase[u, t, b] = float32(int32(v)) * float32(pi / 2^31) for t < n_frames[u], 0.0f beyond.
 * Expected magnitudes are finite and non-negative; for them |p| <= 1/2 up to rounding.  No index is ever computed from a
 * magnitude's value, only from comparisons, so any input bits (NaN, inf, negative) give some phase and never an
 * out-of-range access; a p that is not finite or exceeds 1 in magnitude (only such inputs produce one) counts as 0.
 *
 * Three launches on `stream`, 32 frames per chunk: per (utterance, chunk) the composed map of the chunk's frames
 * (source bin uint16, offset uint32 per bin), per utterance the state at every chunk's start, per (utterance, chunk) the
 * replay that writes the phases.  No workgroup waits for another, no atomics, no memset, no host synchronisation:
 * hipGraph-capturable; every element of d_phase is written exactly once and d_amp is only read.  d_workspace:
 * vc_phase_spsi_workspace_bytes bytes (10 bytes per bin and chunk), 4-byte aligned, contents irrelevant before and after.
 * VC_ERR_INVALID before any launch for a NULL pointer, batch outside [1, 65535], max_frames < 1, n_fft < 4,
 * n_bins != 1 + n_fft/2, n_bins > 65535, hop outside [1, 65535], a short workspace, and for n_bins > 2978: the
 * kernels keep a fill's magnitudes and tables in 64 KiB of LDS at 22 bytes per bin (n_fft up to 5955; the vocoder
 * itself stops at n_fft 4096). */
size_t vc_phase_spsi_workspace_bytes(int32_t batch, int32_t max_frames, int32_t n_bins);
int vc_phase_spsi(const float* d_amp, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_bins,
                  int32_t n_fft, int32_t hop, float* d_phase, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Resampling: what librosa.load(path, cfg['sample_rate']) does to a file of another rate before the reference sees it
 * (test.py:472, ARCTIC_reader.py:233, TIMIT_reader.py:308, TARGET_spk_reader.py:108), for a ragged batch on the device.
 * Added without a version bump: no existing signature moved, a library without these symbols fails to bind them by name.
 *
 * Band-limited interpolation with a Kaiser-windowed sinc, evaluated exactly at every phase (no interpolated table).
 * For integer rates, g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g, fc = rolloff * min(1, up / down):
 *     h(t) = fc * sinc(fc t) * I0(beta * sqrt(1 - u^2)) / I0(beta),  u = t * fc / Z,  |u| < 1, else 0   (t in input samples)
 *     y[m] = sum_{0 <= n < len_in} x[n] * h((m * down - n * up) / up),      0 <= m < len_out = ceil(len_in * up / down)
 * The caller passes the taps of the up-sampled domain, h_taps[k + half] = h(k / up) for |k| <= half (float64, 2*half+1
 * values; audio_lib.resample_taps builds them); the plan rounds them to float32 and stores, per phase p = (m * down) % up,
 * the row of taps k = p + j * up.  VC_ERR_UNSUPPORTED (before any HIP call) when the table exceeds 2^24 floats or the
 * input span of one tile (4 * down + taps per phase, at least) exceeds 16,000 samples of LDS.
 *
 * vc_resample_f32: d_in [batch] rows of max_in samples, row stride ld_in >= max_in; d_lens_in int32 [batch] (NULL =
 * max_in; values are clamped to [0, max_in]); d_out [batch] rows of max_out >= ceil(max_in * up / down) samples, stride
 * ld_out.  One launch, no workspace, no memset, no atomics: every element of every output row up to max_out is written
 * exactly once, zeros from the row's own len_out on.  float32 taps, samples and accumulation; the accumulation is
 * compensated (the rounding error of every product and of every addition is carried in a second float32 word and added
 * at the end), so an output is the float32 rounding of the exact sum of its float32 products, and it runs in a fixed
 * order per output: an utterance's output is bit-identical alone and in any batch.  m * down is formed in 64 bits. */
typedef struct vc_resample_plan vc_resample_plan;
int vc_resample_plan_create(int32_t up, int32_t down, int32_t half, const double* h_taps, vc_resample_plan** out_plan);
void vc_resample_plan_destroy(vc_resample_plan* plan);
int vc_resample_f32(const vc_resample_plan* plan, const float* d_in, const int32_t* d_lens_in, int32_t batch, int32_t max_in,
                    int32_t ld_in, float* d_out, int32_t max_out, int32_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Evaluation: how close a converted utterance is to the target speaker's own recording of the sentence -- mel-cepstral
 * distortion (MCD, in dB) along a dynamic-time-warping (DTW) path, or frame by frame for two conversions of one input.
 * Added without a version bump, like the resampler: no existing signature moved.
 *
 * Cepstra.  For mel [rows, n_mels] (the front-end's M_dB or the decoder's mel output, float32 or bf16):
 *     c[row, d] = sum_m dct[d, m] * mel[row, m],  d = 0 .. n_coef-1,  m ascending, float32 fused multiply-adds.
 * d_dct is [n_coef, n_mels] float32 ON THE DEVICE: the rows first_coef .. first_coef + n_coef - 1 of the orthonormal
 * DCT-II (dct[k, m] = sqrt(2 / n_mels) * cos(pi * k * (2 m + 1) / (2 n_mels)), row 0 scaled by sqrt(1/2): the table of
 * vc_frontend_host_tables), built on the host in float64 and rounded once.  1 <= n_coef <= min(n_mels, 32), n_mels <= 512.
 *
 * Frame distance:  d(i, j) = scale * sqrt(2 * sum_d (ca[i, d] - cb[j, d])^2), the sum over d ascending, fused
 * multiply-adds, a correctly rounded square root.  With mel = M_dB_norm_factor * (20 log10(mel power) - min), the natural
 * logarithm of the mel amplitude is mel * ln 10 / (40 * M_dB_norm_factor) + const, and the textbook
 * (10 / ln 10) * sqrt(2 * sum (delta mc)^2) becomes scale = 1 / (4 * M_dB_norm_factor): 25 for the shipped 0.01.
 *
 * DTW.  D(0, 0) = d(0, 0);  D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)); on exact equality the
 * predecessor is taken in that order (diagonal, up, left).  L(i, j) = 1 + L(predecessor), L(0, 0) = 1.  Per pair:
 * total = D(Fa-1, Fb-1), path_len = L(Fa-1, Fb-1), mcd = total / path_len (float32 division).  band >= 0 allows cell
 * (i, j) iff |j * (Fa-1) - i * (Fb-1)| <= band * max(Fa-1, Fb-1), tested in 64-bit integers; every other cell has
 * D = +inf and L = 0; the end cell is always allowed.  band = -1: no band.  A band that disconnects the end from the
 * start (band = 0 with Fa != Fb, for one) gives total = +inf; path_len and mcd then hold what the recurrence leaves in
 * the end cell and mean nothing, and vc_dtw_backtrack writes no path.
 *
 * vc_dtw_f32: d_ca [batch, max_a, n_coef], d_cb [batch, max_b, n_coef] float32, contiguous; d_len_a / d_len_b int32
 * [batch] ON THE DEVICE, clamped to [1, max]; 1 <= max_a, max_b <= 16,384, n_coef <= 32 (else VC_ERR_UNSUPPORTED);
 * scale finite and > 0.  One launch, one workgroup per pair; no matrix of costs or distances is ever stored: score mode
 * (want_path = 0) uses 16 bytes of workspace per column of B and pair.  want_path = 1 also stores two bits per cell
 * (0 diagonal, 1 up, 2 left; row-major, sixteen columns to a word) and gives bit-identical total / path_len;
 * VC_ERR_UNSUPPORTED when the codes of the batch exceed 2^31 bytes (one pair of 16,384 x 16,384 takes 2^26).
 * vc_dtw_workspace_size: bytes for either mode (host arithmetic only; 0 for a shape the launch would refuse).  The
 * workspace is 16-byte aligned (VC_ERR_INVALID otherwise) and may be exactly that long (VC_ERR_WORKSPACE when shorter);
 * its contents before the launch do not matter.
 * vc_dtw_backtrack: from the workspace a want_path launch filled (same batch, max_a, max_b) and its d_total /
 * d_path_len, d_path [batch, max_a + max_b - 1, 2] int32: the cells (i, j) from (0, 0) to (Fa-1, Fb-1), rows from
 * path_len on filled with -1 (all rows when total is not finite).
 * vc_frame_mcd_f32: mcd = (1 / n) * sum_{i < n} d(i, i), n = min(Fa, Fb): lane t of 256 adds frames t, t + 256, ... in
 * that order and the 256 partial sums are added in a fixed tree.
 *
 * Every result is a function of its own pair alone: bit-identical alone, inside any batch, from run to run and under
 * graph replay.  No atomics.  Every launch is capturable; arguments are checked before any HIP call. */
int vc_mel_cepstra(const void* d_mel, int32_t mel_dtype, int32_t rows, int32_t n_mels, const float* d_dct, int32_t n_coef,
                   float* d_cep, void* stream);
size_t vc_dtw_workspace_size(int32_t batch, int32_t max_a, int32_t max_b, int32_t want_path);
int vc_dtw_f32(const float* d_ca, const float* d_cb, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
               int32_t max_a, int32_t max_b, int32_t n_coef, float scale, int32_t band, int32_t want_path, float* d_total,
               int32_t* d_path_len, float* d_mcd, void* d_workspace, size_t workspace_bytes, void* stream);
int vc_dtw_backtrack(const void* d_workspace, size_t workspace_bytes, const int32_t* d_len_a, const int32_t* d_len_b,
                     const float* d_total, const int32_t* d_path_len, int32_t batch, int32_t max_a, int32_t max_b, int32_t* d_path,
                     void* stream);
int vc_frame_mcd_f32(const float* d_ca, const float* d_cb, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
                     int32_t max_a, int32_t max_b, int32_t n_coef, float scale, float* d_mcd, void* stream);

/* Pitch.  MCD leaves out the gain term and sees the spectral envelope only; the other two figures reported for a pair of
 * utterances are the F0 error and the voiced / unvoiced error along the same path.  Added without a version bump.
 *
 * F0 is YIN (de Cheveigne and Kawahara 2002), steps 2 to 5, on the raw waveform: no pre-emphasis, no amplitude
 * normalisation (the normalised difference does not change under a gain; a power-of-two gain leaves every output bit
 * for bit).  Parameters: sample_rate, hop, the integration length W = frame_length, tau_min = floor(sr / fmax),
 * tau_max = ceil(sr / fmin) (40 and 267 for 400 and 60 Hz at 16 kHz), threshold (0.15).
 *   Frames      F = 1 + len / hop, the front-end's count: frame f of the track and frame f of the mel spectrogram sit at
 *               the same time.  Frame f reads x[s .. s + W + tau_max], s = f * hop - (W + tau_max) / 2, zeros outside
 *               [0, len).
 *   Difference  d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2, tau = 0 .. tau_max + 1: the DIRECT form (the
 *               energy-minus-correlation form cancels where this one adds non-negative terms), j ascending, one chain of
 *               float32 fused multiply-adds per lag.
 *   Normalised  d'(0) = 1, d'(tau) = d(tau) * tau / sum_{k = 1..tau} d(k) (one rounded product, one correctly rounded
 *               division), and 1 where that sum is zero: digital silence gives d' = 1 everywhere.  The running sum is a
 *               scan in a fixed order: inside groups of 64 lags, six steps of lag t adding lag t - 2^k; then the totals
 *               of the groups before this one, added in order.
 *   Pick        the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then on while tau + 1 <= tau_max and
 *               d'(tau + 1) < d'(tau).  None: the frame is unvoiced, f0 = 0.
 *   Refine      a parabola through d'(tau - 1), d'(tau), d'(tau + 1): offset = 0.5 (y0 - y2) / (y0 - 2 y1 + y2) when the
 *               denominator is positive, else 0, clamped to [-0.5, 0.5]; f0 = sample_rate / (tau + offset).
 *   Aperiodicity  min over tau_min <= tau <= tau_max of d'(tau), for every frame, voiced or not.
 * No smoothing, no octave correction in this launch ("Pitch tracking" below decodes a path through several candidates
 * per frame).  Samples are expected to be finite.
 *
 * vc_f0_yin_f32: d_wav [batch] rows of max_len samples, row stride ld >= max_len; d_lens int32 [batch] ON THE DEVICE
 * (NULL = max_len), clamped to [0, max_len]; d_f0, d_aperiodicity [batch, max_frames] float32, max_frames >=
 * 1 + max_len / hop.  One launch, one workgroup per (utterance, tile of up to 16 frames), the tile's samples staged once
 * in at most 64 KB of LDS, one lane per lag; no workspace, no atomics.  Every element of both outputs is written exactly
 * once: f0 = 0 and aperiodicity = 1 from the row's own frame count on.  Limits (VC_ERR_UNSUPPORTED beyond them):
 * batch <= 65,535, max_len <= 2^30 (sample indices stay in int32), frame_length <= 2,048, tau_max <= 1,022 (one lane per
 * lag, 1,024 lanes: fmin >= 15.7 Hz at 16 kHz), hop <= 65,536, max_frames <= 2^30 + 1.
 *
 * vc_f0_metrics_f32: the figures of `batch` pairs of tracks d_f0_a [batch, max_a], d_f0_b [batch, max_b] (0 = unvoiced)
 * with d_len_a / d_len_b int32 [batch] on the device, clamped to [1, max].  The cells are d_path [batch, max_path, 2]
 * int32 with d_path_len [batch] (clamped to [0, max_path]) -- exactly what vc_dtw_backtrack and vc_dtw_f32 write -- or,
 * with d_path = d_path_len = NULL and max_path = 0, the cells (i, i), i < min(len_a, len_b).  A cell outside [0, len_a) x [0, len_b) is skipped and
 * not counted.  Per pair: d_counts [batch, 3] int32 = n_cells, n_both_voiced, n_vuv_mismatch (one side voiced, the other
 * not); d_values [batch, 4] float32 = vuv_error (n_vuv_mismatch / n_cells), f0_rmse_cents
 * (sqrt(mean (1200 log2(fa / fb))^2) over the both-voiced cells), f0_rmse_hz, logf0_corr (Pearson correlation of log2 f0
 * over the both-voiced cells, taken about the means).  NaN where undefined: vuv_error without a cell, the RMSE values
 * without a both-voiced cell, the correlation with fewer than two of them or when one side has the same f0 in all of
 * them.  One workgroup per pair; cells dealt to 256 lanes by stride, sums in float64 added in a fixed tree, rounded to
 * float32 once.  Limits: batch <= 65,535; max_a, max_b, max_path <= 2^30.
 *
 * Both are functions of their own utterance / pair alone, bit-identical alone, in any batch, from run to run and under
 * graph replay; capturable from the first call; arguments are checked before any HIP call. */
int vc_f0_yin_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, float sample_rate,
                  int32_t hop, int32_t frame_length, int32_t tau_min, int32_t tau_max, float threshold, float* d_f0,
                  float* d_aperiodicity, int32_t max_frames, void* stream);
int vc_f0_metrics_f32(const float* d_f0_a, const float* d_f0_b, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
                      int32_t max_a, int32_t max_b, const int32_t* d_path, const int32_t* d_path_len, int32_t max_path,
                      int32_t* d_counts, float* d_values, void* stream);

/* Pitch tracking.  vc_f0_yin_f32 decides every frame alone and takes the FIRST dip of d' below the threshold; where the
 * fundamental is weak the dip at half the period slips under the threshold and the frame is reported an octave high.
 * These two launches keep several candidates per frame and choose among them along the utterance (Viterbi decoding, as
 * in pYIN's second stage, on YIN's own d').  Added without a version bump.
 *
 * Candidates.  Frames, d(tau) and d'(tau) are exactly those of vc_f0_yin_f32 (the same frame count and placement, the
 * direct-form difference, the same order of the running sum: the kernels share that code).  A lag tau in
 * [tau_min, tau_max] is a candidate when d'(tau) < d'(tau - 1) (the left neighbour counts as +inf at tau = tau_min),
 * d'(tau) <= d'(tau + 1) (the right neighbour as +inf at tau = tau_max) and d'(tau) < ceiling; so some lag holding the
 * range minimum is a candidate whenever that minimum is below the ceiling.  The n_cand candidates of lowest d' are kept
 * (on a tie in d' the smaller lag) and stored in ascending lag, each with f0 = sample_rate / (tau + offset) (YIN's
 * clamped parabola, the same arithmetic), pitch = log2(f0) and cost = d'(tau).  Per frame also n, the number of
 * candidates kept, and aperiodicity, the minimum of d' over the range, bit-identical to vc_f0_yin_f32's.  From an
 * utterance's frame count on n = 0 and aperiodicity = 1; slots from n on hold f0 = 0, pitch = 0, cost = 1.  Digital
 * silence (d' = 1 everywhere) gives n = 0 for any ceiling <= 1.
 *
 * vc_f0_candidates_f32: d_wav, d_lens, max_len, ld, sample_rate, hop, frame_length, tau_min, tau_max, max_frames as
 * vc_f0_yin_f32; d_f0, d_pitch, d_cost [batch, max_frames, n_cand] float32; d_n [batch, max_frames] int32;
 * d_aperiodicity [batch, max_frames] float32.  vc_f0_yin_f32's tiling; after d' is in LDS each lane flags a local
 * minimum, and the n_cand lowest are taken by repeated arg-min over (d', lag) in a fixed order (no atomics).  Every
 * output element is written exactly once.  Limits: those of vc_f0_yin_f32 and 1 <= n_cand <= 15; ceiling finite and > 0.
 *
 * Decoding.  S = n_cand + 1 states per frame: state 0 is unvoiced with local cost unvoiced_cost, state k >= 1 is
 * candidate k - 1 with local cost cost[k - 1]; a state beyond n[f] is absent (cost +inf).  Transition t(i, j): 0 between
 * unvoiced and unvoiced, switch_cost between unvoiced and voiced either way, jump_cost * |pitch_i - pitch_j| between two
 * voiced states.  In float32, in this association order, nothing fused:
 *     delta_0(j) = c_0(j);    delta_f(j) = min_i (delta_{f-1}(i) + t(i, j)) + c_f(j),  the lowest i among equals;
 * after every frame m_f = min_j delta_f(j) is subtracted from every state and added into a float64 total (delta stays at
 * the size of the transition costs however long the utterance is).  The last state is the lowest j of minimal delta;
 * the path is read back from the stored predecessors.  With jump_cost = switch_cost = 0 and unvoiced_cost = threshold a
 * frame is voiced exactly when its aperiodicity is below the threshold: YIN's decision.
 *
 * vc_f0_viterbi_f32: d_pitch, d_cost [batch, max_frames, n_cand] float32 and d_n [batch, max_frames] int32 (clamped to
 * [0, n_cand]) as vc_f0_candidates_f32 writes them; d_frames int32 [batch] ON THE DEVICE, the frame counts (NULL =
 * max_frames), clamped to [0, max_frames].  d_state [batch, max_frames] int32: 0 unvoiced, k candidate k - 1, -1 from
 * the frame count on; d_total [batch] float32, the float64 total rounded once (0 without a frame); with d_cand_f0
 * [batch, max_frames, n_cand] also d_f0 [batch, max_frames] = the chosen candidate's f0, 0 where unvoiced or beyond the
 * frame count (pass both or NULL for both).  One wave per utterance; the lattice is staged through LDS in tiles of
 * vc_f0_viterbi_tile() frames, two buffers; the predecessors are 4 bits per state, 8 bytes per frame, in d_workspace
 * (8-byte aligned, vc_f0_viterbi_workspace_size bytes: host arithmetic only, 0 for a shape the launch would refuse).
 * Every output element is written exactly once; no atomics, no memset.  The three costs must be finite and not negative
 * (VC_ERR_INVALID).  Limits (VC_ERR_UNSUPPORTED): batch <= 65,535, max_frames <= 2^30 + 1, n_cand <= 15.
 *
 * Both are functions of their own utterance alone, bit-identical alone, in any batch, from run to run and under graph
 * replay; capturable from the first call; arguments are checked before any HIP call. */
int vc_f0_candidates_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, float sample_rate,
                         int32_t hop, int32_t frame_length, int32_t tau_min, int32_t tau_max, float ceiling, int32_t n_cand,
                         float* d_f0, float* d_pitch, float* d_cost, int32_t* d_n, float* d_aperiodicity, int32_t max_frames,
                         void* stream);
int32_t vc_f0_viterbi_tile(void);
size_t vc_f0_viterbi_workspace_size(int32_t batch, int32_t max_frames, int32_t n_cand);
int vc_f0_viterbi_f32(const float* d_pitch, const float* d_cost, const int32_t* d_n, const int32_t* d_frames, int32_t batch,
                      int32_t max_frames, int32_t n_cand, float unvoiced_cost, float jump_cost, float switch_cost,
                      const float* d_cand_f0, int32_t* d_state, float* d_f0, float* d_total, void* d_workspace,
                      size_t workspace_bytes, void* stream);

/* Speech activity.  The scores above run over every frame, silence included; these five launches answer "where is the
 * speech" on the device, so that the DTW, the MCD and the F0 figures can be taken over speech frames only.  Added without
 * a version bump.
 *
 *   Frame energy  F = 1 + len / hop frames, the front-end's and the tracker's count.  e[f] = sum_{j < W} x[s + j]^2,
 *                 s = f * hop - W / 2, zeros outside [0, len); 0 from frame F on.  Order: lane l of 64 adds the squares
 *                 of samples j = l, l + 64, l + 128, ... of the frame in one chain of float32 fused multiply-adds; the
 *                 64 partial sums are then added in a butterfly (every lane adds the sum of lane l ^ 32, then l ^ 16, ...
 *                 l ^ 1).  A frame's energy depends on its own W samples alone.
 *   Raw decision  mode 1 ('energy'): e[f] > 0 and e[f] > float32(ratio * max_f e[f]), ratio = 10^(-top_db / 10) computed
 *                 on the host in float64 and rounded once (1e-4 for the default 40 dB); a power-of-two gain changes
 *                 nothing.  mode 2 ('voiced'): f0[f] > 0, the tracker's output.  mode 3: both.
 *   Smoothing     integer run-length work.  First every run of inactive frames of length <= max_gap with an active frame
 *                 on both sides becomes active; then every run of active frames shorter than min_run becomes inactive
 *                 (runs touching the first or the last frame count with their own length).  max_gap = 0 and
 *                 min_run <= 1 change nothing.
 *   Compaction    index[k] = the frame number of the k-th active frame, ascending; n_active their count; n_kept =
 *                 n_active, except that an utterance without an active frame (digital silence, 'voiced' on noise) keeps
 *                 all its F frames (index = 0 .. F-1, n_kept = F: vc_dtw_f32 needs lengths in [1, F]; the caller reads
 *                 the case off n_active == 0).  index is -1 from n_kept on.  A second mask is ANDed in first over the
 *                 frames i < F = min(F_a, F_b); frames beyond are inactive, and the fallback keeps those F frames.
 *   Intervals     the maximal runs of active frames as [start, end) pairs, ascending, n_intervals of them, at most
 *                 (max_a + 1) / 2; unused rows are -1; none when n_active == 0.
 *
 * vc_frame_energy_f32: d_wav, d_lens, max_len, ld as vc_f0_yin_f32; d_energy [batch, max_frames] float32, max_frames >=
 * 1 + max_len / hop, every element written once.  One workgroup per (utterance, tile of vc_frame_energy_tile(hop,
 * frame_length) frames: 64, halved until the tile's frame_length + (tile - 1) hop samples fit 64 KB of LDS), one wave per
 * frame.  The only launch that reads the waveform.  Limits: batch <= 65,535, max_len <= 2^30, frame_length <= 8,192,
 * hop <= 65,536.  vc_frame_energy_tile is host arithmetic (0 for values the launch would refuse).
 * vc_activity_mask: d_energy (modes 1, 3) and d_f0 (modes 2, 3) [batch, max_frames] float32, d_n_frames int32 [batch] on
 * the device, clamped to [1, max_frames]; d_mask [batch, max_frames] uint8, 0 from the row's frame count on.  The
 * pointer of a mode that does not use it may be NULL.  In the energy modes ratio must lie in (0, 1): 0, 1 or a NaN are
 * refused with VC_ERR_INVALID (a ratio of 0 would be "e > 0" alone).  One workgroup per utterance; max_frames <= 16,384.
 * vc_mask_compact: d_mask_a [batch, max_a] with d_frames_a; d_mask_b [batch, max_b] with d_frames_b, or NULL, NULL, 0.
 * d_index [batch, max_a], d_n_active, d_n_kept, d_n_intervals [batch], d_intervals [batch, (max_a + 1) / 2, 2], int32.
 * One workgroup per utterance, positions by a sum scan in a fixed order; max_a, max_b <= 16,384.
 * vc_compact_rows_f32: d_dst[b, k, :] = d_src[b, d_index[b, k], :] for k < min(d_n_kept[b], index_frames), zeros beyond
 * (a negative d_n_kept counts as 0), and zeros for an index outside [0, src_frames);
 * d_src [batch, src_frames, n_cols], d_index [batch, index_frames], d_dst [batch, dst_frames, n_cols].  The indices live
 * on the device (vc_gather_rows takes a host-built list of the whole batch).  n_cols <= 4,096.
 * vc_path_map: d_path_out[b, p] = (d_index_a[b, i], d_index_b[b, j]) for the cell (i, j) = d_path_in[b, p], p <
 * d_path_len[b] (clamped to [0, max_path]); (-1, -1) beyond, and for a cell outside [0, max_a) x [0, max_b).  d_path_in
 * NULL: the cells (p, p).
 * d_path_out may be d_path_in.  After it the path indexes the original frames, and vc_f0_metrics_f32 runs unchanged on
 * the original tracks and lengths.
 *
 *
 * Speech-level gain.  The front-end scales an utterance to a mean |x| of mean_abs_amp_norm over ALL its samples and floors
 * the mel power, so the mel of the same speech depends on how much silence surrounds it (2 s of speech with 2.8 s of
 * silence added: cells 15 dB up against a fixed floor, 8.8 dB of MCD between identical speech).  The masked waveform-level
 * scores therefore take the gain over the speech samples: sample i belongs to frame min((i + hop / 2) / hop, F - 1), and
 *     gain = target * n / sum |x[i]|  over the n samples of active frames (all samples when no frame is active; 1 when
 *     they are all zero),
 * and run the front-end on gain * x with its own normalisation off (mean_abs_amp_norm = 1).
 * vc_speech_gain_f32: d_wav, d_lens, max_len, ld as above; d_mask [batch, max_frames] and d_n_active [batch] from the two
 * launches above; d_gain [batch] float32.  One workgroup per utterance; lane t of 1,024 adds samples t, t + 1024, ... in
 * float64, the partial sums are added in a fixed tree, the quotient is rounded to float32 once.
 * vc_scale_rows_f32: d_out[b, i] = d_gain[b] * d_wav[b, i] for i < len, 0 beyond; d_out [batch, max_len] contiguous.
 *
 * No atomics, no hand-off between workgroups, no memset, no workspace; every output is a function of its own utterance
 * alone, bit-identical alone, in any batch, from run to run and under graph replay; capturable from the first call. */
int vc_frame_energy_tile(int32_t hop, int32_t frame_length);
int vc_frame_energy_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, int32_t hop,
                        int32_t frame_length, float* d_energy, int32_t max_frames, void* stream);
int vc_activity_mask(const float* d_energy, const float* d_f0, const int32_t* d_n_frames, int32_t batch, int32_t max_frames,
                     int32_t mode, float ratio, int32_t max_gap, int32_t min_run, uint8_t* d_mask, void* stream);
int vc_mask_compact(const uint8_t* d_mask_a, const int32_t* d_frames_a, int32_t max_a, const uint8_t* d_mask_b,
                    const int32_t* d_frames_b, int32_t max_b, int32_t batch, int32_t* d_index, int32_t* d_n_active, int32_t* d_n_kept,
                    int32_t* d_intervals, int32_t* d_n_intervals, void* stream);
int vc_compact_rows_f32(const float* d_src, int32_t src_frames, const int32_t* d_index, int32_t index_frames, const int32_t* d_n_kept,
                        int32_t batch, int32_t n_cols, float* d_dst, int32_t dst_frames, void* stream);
int vc_path_map(const int32_t* d_path_in, const int32_t* d_path_len, int32_t batch, int32_t max_path, const int32_t* d_index_a,
                int32_t max_a, const int32_t* d_index_b, int32_t max_b, int32_t* d_path_out, void* stream);
int vc_speech_gain_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, int32_t hop,
                       const uint8_t* d_mask, const int32_t* d_n_active, int32_t max_frames, float target, float* d_gain,
                       void* stream);
int vc_scale_rows_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, const float* d_gain,
                      float* d_out, void* stream);

/* Content.  MCD sees the spectral envelope and the F0 figures the prosody; the third question asked of a conversion is
 * whether it still says the same thing.  The encoder is a frame-level phoneme recogniser, so the answer is taken from the
 * posteriorgrams (PPG) [frames, C] of the two sides: their frame-level agreement along a set of cells, and the edit
 * distance of the phoneme sequences read off them.  Added without a version bump.
 *
 * vc_ppg_metrics_f32: d_ppg_a [batch, max_a, C], d_ppg_b [batch, max_b, C] float32, contiguous; d_len_a / d_len_b int32
 * [batch] on the device, clamped to [1, max].  The cells are taken exactly as vc_f0_metrics_f32 takes them: d_path
 * [batch, max_path, 2] int32 with d_path_len [batch], as vc_dtw_backtrack writes them, or, with both NULL and max_path = 0,
 * the cells (i, i), i < min(len_a, len_b); a cell outside [0, len_a) x [0, len_b) is skipped and not counted.
 * d_class_map: int32 [C] on the device or NULL (the identity), applied to the arg-max before the comparison.  Per cell,
 * with p = a[i, :], q = b[j, :], m = (p + q) / 2:
 *     js = 0.5 * sum_c (p log2(p / m) + q log2(q / m))        (the Jensen-Shannon divergence in bits)
 * where a term whose p (or q) is <= 0 contributes 0; posteriors are taken as given, not renormalised, and are expected to
 * be finite.  The arithmetic of a cell is float64: the float32 operands widened, float64 division and log2.  The arg-max
 * takes the lowest index on equality.  Per pair: d_counts [batch, 2] int32 = n_cells, n_agree (cells where
 * map[argmax p] == map[argmax q]); d_values [batch, 2] float32 = frame_agreement (n_agree / n_cells) and js_mean (the
 * mean of js over the counted cells, in [0, 1] for distributions); both NaN without a cell.  Sums are float64 added in a
 * fixed tree -- a lane adds its classes c = l, l + 64, ... ascending, the 64 lanes of a cell are added in a butterfly, a
 * wave adds its cells k = w, w + 16, ... ascending, the sixteen waves are added in order -- and rounded to float32 once.
 * Identical inputs give js_mean == 0 exactly (p / m = 1).  One workgroup per pair, one wave per cell.  Limits
 * (VC_ERR_UNSUPPORTED beyond them): 1 <= C <= 256; batch <= 65,535; max_a, max_b, max_path <= 2^30.
 *
 * vc_phn_segments: d_ppg [batch, max_frames, C] float32; d_n_frames int32 [batch] on the device, clamped to
 * [0, max_frames]; min_run >= 1; d_class_map int32 [C] on the device or NULL, values in [-1, C), -1 = "drop this class".
 * In this order, not iterated:
 *   1. l[f] = argmax_c ppg[f, c], the lowest index on equality; with a map l[f] = map[l[f]] (-1 is a label like any other
 *      at this point);
 *   2. runs are the maximal stretches of equal l;
 *   3. runs shorter than min_run frames are removed;
 *   4. among the survivors, neighbours with the same label merge: the segment starts at the first run's start and ends at
 *      the last run's end;
 *   5. segments labelled -1 are then removed; their neighbours do not merge ("a pau a" stays two "a").
 * d_labels, d_start, d_end [batch, max_frames] int32 (end exclusive), all three -1 from the row's own count on; d_n_seg
 * [batch].  Every output element is written exactly once.  One workgroup of 1,024 lanes per utterance; the frames go
 * through in tiles of vc_phn_segments_tile() = 1,024 with the carried state in registers, the positions by block-wide
 * prefix scans in a fixed order; no workspace.  Limits: C <= 256; max_frames <= 2^30; batch <= 65,535.
 *
 * vc_edit_distance_i32: d_seq_a [batch, max_a], d_seq_b [batch, max_b] int32; d_n_a / d_n_b int32 [batch] on the device,
 * clamped to [0, max].  Unit costs: E(i, 0) = i (all deletions), E(0, j) = j (all insertions),
 *     E(i, j) = min(E(i-1, j-1) + [a_i != b_j], E(i-1, j) + 1, E(i, j-1) + 1);
 * on equality the predecessor is taken in the order diagonal, up, left (the DTW's order).  Every cell carries (n_match,
 * n_sub, n_del, n_ins) from its chosen predecessor: a diagonal step adds a match or a substitution, an up step a deletion
 * (a symbol of A without a partner), a left step an insertion -- as L rides with D in vc_dtw_f32, so there is no back-track
 * and no matrix.  d_counts [batch, 5] int32 = dist, n_match, n_sub, n_del, n_ins, with dist = n_sub + n_del + n_ins and
 * n_match + n_sub + n_del = n_a; d_per [batch] float32 = dist / n_a (A is the reference), NaN when n_a = 0.  Integer
 * arithmetic throughout: bit-exact against the definition.  One launch, one workgroup (one wave) per pair, the wavefront
 * over anti-diagonals, vc_edit_distance_rows() = 256 symbols of A per pass; the workspace (vc_edit_distance_workspace_bytes:
 * host arithmetic, 0 for a shape the launch would refuse) holds 32 bytes per column of B and pair, the row between two
 * passes.  Limits: max_a, max_b <= 16,384; batch <= 65,535.
 *
 * All three are functions of their own pair / utterance alone, bit-identical alone, in any batch, from run to run and
 * under graph replay; no atomics; capturable from the first call; arguments are checked before any HIP call. */
int vc_ppg_metrics_f32(const float* d_ppg_a, const float* d_ppg_b, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
                       int32_t max_a, int32_t max_b, int32_t n_classes, const int32_t* d_path, const int32_t* d_path_len,
                       int32_t max_path, const int32_t* d_class_map, int32_t* d_counts, float* d_values, void* stream);
int vc_phn_segments_tile(void);
int vc_phn_segments(const float* d_ppg, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_classes,
                    int32_t min_run, const int32_t* d_class_map, int32_t* d_labels, int32_t* d_start, int32_t* d_end,
                    int32_t* d_n_seg, void* stream);
int vc_edit_distance_rows(void);
size_t vc_edit_distance_workspace_bytes(int32_t batch, int32_t max_a, int32_t max_b);
int vc_edit_distance_i32(const int32_t* d_seq_a, const int32_t* d_seq_b, const int32_t* d_n_a, const int32_t* d_n_b, int32_t batch,
                         int32_t max_a, int32_t max_b, int32_t* d_counts, float* d_per, void* d_workspace, size_t workspace_bytes,
                         void* stream);

/* Speaker.  The fourth question asked of a conversion: does it sound like the target speaker, and no longer like the
 * source?  The text-independent answer needs no parallel sentence and no pretrained model: a diagonal-covariance
 * Gaussian mixture fitted on the cepstra of many speakers (the universal background model, UBM), the same mixture with
 * its means MAP-adapted to one speaker, and the mean per-frame log-likelihood ratio (LLR) of an utterance between the
 * two (Reynolds, Quatieri and Dunn 2000).  Added without a version bump.
 *
 * Limits (VC_ERR_UNSUPPORTED beyond them): components 1 <= M <= 256; feature width 1 <= D <= 64; batch <= 65,535;
 * max_frames * D <= 2^30; groups <= 4,096; models of one table <= 4,097 (4,096 speakers and the UBM).  Lengths d_len int32 [batch] ON THE DEVICE, clamped to
 * [0, max_frames]; masks uint8 [batch, max_frames] on the device or NULL (every frame); a frame is KEPT when its mask is
 * set and it lies below the length.  float32 arithmetic unless said otherwise.  A d_len outside [0, max_frames], of any
 * magnitude, is clamped and never refused, in all four launches that take it (features, loglik, score, accumulate); features,
 * cepstra, ll and mask bytes from len on are not read.
 *
 * vc_spk_features_f32: d_cep [batch, max_frames, n_coef] (what vc_mel_cepstra writes), n_coef <= 32; d_feat
 * [batch, max_frames, D], D = n_coef * (1 + deltas).  Columns 0 .. n_coef-1 are the cepstra; with deltas = 1 columns
 * n_coef .. 2 n_coef - 1 are
 *     delta[t] = ((c[t+1] - c[t-1]) + 2 (c[t+2] - c[t-2])) / 10,  indices clamped to [0, len-1]
 * (two rounded differences, one fused multiply-add, one correctly rounded division; over ALL frames below len, masked or
 * not).  With cmn = 1 the mean of every column over the kept frames is subtracted from all rows below len: the sum is
 * float64 in a fixed order -- lane r of four adds the kept frames r, r + 4, ... ascending, the four partial sums are added
 * in the order ((0 + 1) + 2) + 3 --, the quotient is rounded to float32 once.  Without a kept frame nothing is
 * subtracted.  Rows from len on are zeros.  One workgroup per utterance.
 *
 * The model.  d_w [M], d_mu [n_models, M, D], d_var [M, D]: weights and variances are shared by all models (MAP adaptation
 * here moves means only; model 0 is by convention the UBM).  vc_gmm_prepare_f32 writes the table the other launches
 * read, vc_gmm_table_floats(n_models, M, D) = (n_models + 1) M D + M floats: the means transposed to [model][d][m],
 * 1 / var [d][m] (the float64 quotient of the widened variance, rounded once) and
 *     c_m = log w_m - 0.5 * sum_d log(2 pi var_md)         (float64, d ascending, rounded once).
 * A weight of exactly 0 gives c_m = -inf: that component adds nothing to any ll and has responsibility 0 for every frame (no
 * NaN follows from it as long as one weight is positive).
 *
 * vc_gmm_loglik_f32: per frame x of utterance b, with the means of model d_model[b] (clamped to [0, n_models)):
 *     l_m = c_m - 0.5 * sum_d (x_d - mu_md)^2 * (1 / var_md)    the DIRECT form: the expanded x^2 a - 2 x b product
 *                                                              cancels for narrow components.  d ascending; per term one
 *                                                              rounded difference, one rounded square, one fused
 *                                                              multiply-add
 *     ll  = max_m l_m + log sum_m exp(l_m - max)               the sum: lane l of 64 adds components l, l + 64, ...
 *                                                              ascending, the lanes are added in a butterfly
 * d_ll [batch, max_frames], 0 from len on.  d_model_b / d_ll_b: the same for a second model per utterance, or both NULL;
 * the two passes share one read of the features.  One workgroup per (utterance, tile of vc_gmm_tile_frames() = 32
 * frames).  A frame's ll is a function of the frame and its model alone.
 *
 * vc_gmm_score_f32: d_n_frames [batch] int32 = the kept frames; d_values [batch, 3] float32 = ll_a, ll_b (the means of
 * d_ll_a, d_ll_b over the kept frames) and llr = ll_a - ll_b (the difference of the two float64 means, rounded once).
 * Lane t of 256 adds the kept frames t, t + 256, ... in that order in float64, the 256 partial sums are added in a fixed
 * tree (lane t adds lane t + 128, then t + 64, ... t + 1), each figure is rounded once.  No kept frame: n_frames = 0 and
 * NaN figures.  d_ll_b NULL: ll_b and llr are NaN.
 *
 * vc_gmm_accumulate_f32: the fused E-step.  d_group [batch] int32 in [0, n_groups), or any other value (negative, n_groups,
 * 0x7fffffff: of any magnitude) to leave the utterance out.  d_ll is vc_gmm_loglik_f32's output for model `model` of the
 * table.  In FLOAT64:
 *     N [n_groups, M], S1, S2 [n_groups, M, D] = the sums of gamma, gamma x, gamma x^2 over the kept frames of the group's
 *     utterances, gamma = exp(l_m - ll) (float32, l_m as above);  L [n_groups] = the sum of ll over the same frames.
 * KEPT FRAMES ONLY: a frame the mask drops contributes nothing to N, S1, S2 or L whatever its features and its ll hold (inf
 * and NaN included); frames from len on are not read at all.
 * gamma is formed and folded into the sums; no [frames, M] array exists.  Grid = (chunks of 64 components) x
 * (P = vc_gmm_partitions(n_groups) = max(1, 128 / n_groups) frame partitions) x n_groups: constants and arguments, never
 * a property of the device.  Tile k of utterance b goes to partition (b + k) mod P; a partition walks its utterances
 * and tiles ascending and adds frame by frame; the P partial sums of an element meet in the order 0 .. P - 1 in a
 * second launch: bit-identical from run to run and under graph replay.  Every output element is written once (zeros
 * for a group without utterances).  Workspace: vc_gmm_workspace_bytes(n_groups, M, D) =
 *     n_groups * P * ceil(M / 64) * (64 (1 + 2 D) + 1) * 8 bytes rounded up to 256, and 0 when P = 1 (n_groups > 64: the
 *     workgroups write the outputs themselves);
 * independent of the number of frames, 33,820,672 bytes at most (n_groups = 1, M = 256, D = 64).  Too small:
 * VC_ERR_WORKSPACE.  The workspace may be exactly that long, must be 8-byte aligned (VC_ERR_INVALID otherwise) and need not be
 * cleared: every word read was written by the same call.  Where the query returns 0 it may be NULL with 0 bytes.
 *
 * vc_gmm_update_f32: one launch, elementwise, float64 arithmetic on the float64 statistics, each output rounded once.
 *   mode 0 (EM, n_groups = 1): w_m = max(N_m / sum_k N_k, 2^-40) -- NOT renormalised after the floor (the sum over k
 *     ascending; 2^-40 when there is no frame at all); mu = S1 / N; var = max(S2 / N - mu^2, d_var_floor[d]) with the
 *     unrounded mu.  A component with N_m < min_count keeps d_mu_in and d_var_in (its weight is still updated).
 *   mode 1 (MAP): alpha = N_gm / (N_gm + relevance); mu_g = alpha * (S1_gm / N_gm) + (1 - alpha) * mu_in, d_mu_in [M, D] the
 *     UBM's means, d_mu_out [n_groups, M, D].  N_gm = 0 gives mu_in exactly: a group without utterances returns the UBM's
 *     means bit for bit.  d_S2, d_var_in, d_var_floor, d_w_out, d_var_out are not read and may be NULL.
 *
 * The score figures of an utterance are a function of that utterance and its model alone: bit-identical alone and in any
 * batch.  No atomics, no memset, no host synchronisation, no allocation; every launch is capturable; arguments are
 * checked before any HIP call. */
int vc_gmm_tile_frames(void);
int vc_gmm_partitions(int32_t n_groups);
size_t vc_gmm_table_floats(int32_t n_models, int32_t M, int32_t D);
size_t vc_gmm_workspace_bytes(int32_t n_groups, int32_t M, int32_t D);
int vc_spk_features_f32(const float* d_cep, const int32_t* d_len, const uint8_t* d_mask, int32_t batch, int32_t max_frames,
                        int32_t n_coef, int32_t deltas, int32_t cmn, float* d_feat, void* stream);
int vc_gmm_prepare_f32(const float* d_w, const float* d_mu, const float* d_var, int32_t n_models, int32_t M, int32_t D, float* d_table,
                       void* stream);
int vc_gmm_loglik_f32(const float* d_feat, const int32_t* d_len, int32_t batch, int32_t max_frames, int32_t D, const float* d_table,
                      int32_t n_models, int32_t M, const int32_t* d_model, float* d_ll, const int32_t* d_model_b, float* d_ll_b,
                      void* stream);
int vc_gmm_score_f32(const float* d_ll_a, const float* d_ll_b, const int32_t* d_len, const uint8_t* d_mask, int32_t batch,
                     int32_t max_frames, int32_t* d_n_frames, float* d_values, void* stream);
int vc_gmm_accumulate_f32(const float* d_feat, const float* d_ll, const int32_t* d_len, const uint8_t* d_mask, const int32_t* d_group,
                          int32_t batch, int32_t max_frames, int32_t D, const float* d_table, int32_t n_models, int32_t M, int32_t model,
                          int32_t n_groups, double* d_N, double* d_S1, double* d_S2, double* d_L, void* d_workspace,
                          size_t workspace_bytes, void* stream);
int vc_gmm_update_f32(int32_t mode, const double* d_N, const double* d_S1, const double* d_S2, int32_t n_groups, int32_t M, int32_t D,
                      const float* d_mu_in, const float* d_var_in, const float* d_var_floor, float min_count, float relevance,
                      float* d_w_out, float* d_mu_out, float* d_var_out, void* stream);

/* Alignment.  "Content" reads a phoneme sequence OFF the posteriors; forced alignment goes the other way: the sequence is
 * KNOWN (a transcript) and the question is where each of its states lies in the frames.  An exact dynamic programme over
 * the given states, left to right, with three moves: stay, advance, and skip one state that is marked optional (the
 * silence between two words).  Added without a version bump.
 *
 * Inputs, per utterance b, all on the device: d_score [batch, max_frames, C] float32, the emission score of class c at
 * frame t (callers pass log-posteriors; finite or -inf); d_seq [batch, max_seq] int32, the expected classes; d_opt
 * [batch, max_seq] uint8 or NULL (no state optional), non-zero = the state may be skipped; d_n_frames, d_n_seq int32
 * [batch], clamped to [0, max]: F and S.
 *
 *   Emission    e(t, s) = score[b, t, seq[s]], and -inf when seq[s] lies outside [0, C).  No address is formed from an
 *               unchecked data value.
 *   Recurrence  float32; every operation is one IEEE addition or a compare-select.
 *               D(0, s) = e(0, s) for s = 0, and for s = 1 iff opt[0]; -inf for every other s.
 *               D(t, s) = e(t, s) + best, where best starts as D(t-1, s) (stay, code 0), is replaced by D(t-1, s-1)
 *               (advance, code 1) iff that is strictly greater, and is then replaced by D(t-1, s-2) (skip, code 2) iff
 *               opt[s-1] is set and that is strictly greater.  The strict > in exactly this order is the tie rule (stay
 *               before advance before skip) and the NaN rule (a comparison with a NaN is false).
 *   End         final = S-1; final = S-2 instead iff S >= 2, opt[S-1] is set and D(F-1, S-2) > D(F-1, S-1).
 *               total = D(F-1, final).  The utterance is INFEASIBLE when F == 0, S == 0 or total == -inf.
 *   Path        read back from the codes, mechanically, from (F-1, final): at frame t >= 1 in state s the state of frame
 *               t-1 is s - code(t, s).  (On finite and -inf scores a feasible path ends in a state D(0, .) admits; with a
 *               NaN among the scores the walk is still carried out as written and may end elsewhere.)
 *
 * Outputs, every element written exactly once per call (no memset, no atomics):
 *   d_frame_state [batch, max_frames] int32   the state of every frame; -1 from F on and when infeasible
 *   d_start, d_end [batch, max_seq] int32     first frame and one past the last frame of every visited state; -1 for a
 *                                             skipped state, from S on and when infeasible
 *   d_seg_score [batch, max_seq] float32      the mean of e(t, s) over the state's own frames: the emissions widened to
 *                                             float64, added in frame order, divided by the count (float64), rounded once
 *                                             to float32; NaN where start is -1
 *   d_total [batch] float32                   -inf when infeasible
 *   d_n_visited [batch] int32                 the number of states with start >= 0
 * There is no multiplication anywhere, so nothing can be contracted; additions, the float64 division and the conversions
 * are correctly rounded: the device equals the float32 restatement of tests/align_ref.py BIT FOR BIT in every output, with
 * one exception that is named here: a NaN is a NaN -- the sign and payload bits of a NaN result (possible only when the
 * scores hold a NaN or +inf) are not specified.
 *
 * Two launches on the caller's stream.  Forward: one workgroup of one wave per utterance; a lane owns K = 1, 2, 4, 8 or 16
 * consecutive states (the least such K with 64 K >= max_seq) with their D in registers; the two values a lane needs from
 * its left neighbour come by shuffles; no LDS, no barrier; the emissions are gathered four frames ahead; the two-bit
 * codes of 16 frames make one 32-bit word per state.  Back-track: one workgroup per utterance; one lane walks the codes,
 * then one lane per state writes that state's frames, boundaries and mean.  d_workspace (4-byte aligned):
 *     vc_align_workspace_bytes = align256(4 batch) + align256(batch * ceil(max_frames / 16) * max_seq * 4)
 * (host arithmetic only; 0 for a shape the launch would refuse; too small: VC_ERR_WORKSPACE).  Limits (VC_ERR_UNSUPPORTED
 * beyond them): max_seq <= 1,024; batch <= 65,535; C <= 65,535; max_frames such that the workspace stays below 2^31 bytes.
 * A function of its own utterance alone: bit-identical alone, in any batch, from run to run and under graph replay;
 * lengths are read on the device; capturable from the first call; arguments are checked before any HIP call. */
size_t vc_align_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_seq);
int vc_align_f32(const float* d_score, const int32_t* d_seq, const uint8_t* d_opt, const int32_t* d_n_frames, const int32_t* d_n_seq,
                 int32_t batch, int32_t max_frames, int32_t max_seq, int32_t n_classes, int32_t* d_frame_state, int32_t* d_start,
                 int32_t* d_end, float* d_seg_score, float* d_total, int32_t* d_n_visited, void* d_workspace, size_t workspace_bytes,
                 void* stream);

/* Full-sum alignment: the DISTRIBUTION over the paths of the same lattice, where vc_align_f32 gives the best path.  Added
 * without a version bump.  Inputs exactly as vc_align_f32's (d_score finite or -inf; d_opt may be NULL), the lattice
 * exactly as above: e(t, s) = score[t, seq[s]], -inf for a class outside [0, C); moves stay, advance, and skip one state
 * s-1 iff opt[s-1]; start in state 0, or state 1 iff opt[0]; end in state S-1, or S-2 iff S >= 2 and opt[S-1].  With
 * lse the logarithm of the sum of the exponentials (-inf terms drop out; of nothing but -inf: -inf):
 *
 *   la(0, s)    = e(0, s) on the admitted start states, -inf elsewhere
 *   la(t, s)    = e(t, s) + lse(la(t-1, s), la(t-1, s-1), [opt[s-1]] la(t-1, s-2))
 *   lb(F-1, s)  = 0 on the admitted end states, -inf elsewhere
 *   lb(t, s)    = lse(lb(t+1, s) + e(t+1, s), lb(t+1, s+1) + e(t+1, s+1), [opt[s+1]] lb(t+1, s+2) + e(t+1, s+2))
 *   log_z       = lse over the end states of la(F-1, .)        (the log of the sum over ALL admissible paths of the
 *                                                               product of their frames' exp(e))
 *   gamma(t, s) = exp(la(t, s) + lb(t, s) - log_z)             (the posterior probability of state s at frame t)
 *   Gamma(t, c) = sum over s with seq[s] = c of gamma(t, s)    (with y the logits and e = log_softmax(y):
 *                                                               d(-log_z)/dy = softmax(y) - Gamma)
 *   occ(s)      = sum over t of gamma(t, s)                    (the expected number of frames of state s)
 *
 * The utterance is INFEASIBLE iff F == 0, S == 0 or log_z == -inf.  tests/fullsum_ref.py restates this in float64.
 *
 * Outputs, every element written exactly once per call (no memset):
 *   d_log_z [batch] float32                          -inf when infeasible
 *   d_class_post [batch, max_frames, C] float32      Gamma; all zeros from frame F on and when infeasible
 *   d_state_post [batch, max_frames, max_seq] float32, or NULL: gamma; zeros outside the utterance (frames from F on,
 *                                                    states from S on, infeasible)
 *   d_occ [batch, max_seq] float32                   zeros from S on and when infeasible
 * No output is NaN for any finite-or-(-inf) input.
 *
 * Arithmetic: float32 in the log domain; after each frame the row's maximum over the states is subtracted (forward: and
 * added to a float64 sum, from which log_z is rounded once), so nothing overflows or underflows at any length and mass in
 * states that cannot reach the end costs nothing.  gamma is normalised over the states of its frame, exp(A + B - max) /
 * sum; Gamma is accumulated in 2^-30 fixed point with integer additions, so it is a multiple of 2^-30, independent of the
 * order in which the states of one class arrive, and carries up to S 2^-31 of quantisation on top of gamma's error; occ
 * adds gamma from the last frame to the first.  On scores that are 0 along one admissible path and -inf elsewhere every
 * output is exact (log_z = 0, gamma and Gamma 0 or 1, occ the durations).
 *
 * Two launches on the caller's stream with vc_align_f32's geometry (one wave per utterance, K = 1, 2, 4, 8 or 16
 * consecutive states per lane, the least K with 64 K >= max_seq; neighbours by shuffles; emissions gathered four frames
 * ahead with a clamped frame index; no address from an unchecked class).  Forward stores the shifted rows in d_workspace
 * (4-byte aligned):
 *     vc_fullsum_workspace_bytes = align256(batch * max_frames * max_seq * 4)
 * (host arithmetic only; 0 for a shape the launch would refuse; too small: VC_ERR_WORKSPACE).  Limits (VC_ERR_UNSUPPORTED
 * beyond them): max_seq <= 1,024; batch <= 65,535; C <= 4,096 (the Gamma row lives in LDS); the workspace below 2^31
 * bytes.  A function of its own utterance alone: bit-identical alone, in any batch, from run to run and under graph
 * replay; lengths are read on the device; capturable from the first call; arguments are checked before any HIP call. */
size_t vc_fullsum_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_seq);
int vc_fullsum_f32(const float* d_score, const int32_t* d_seq, const uint8_t* d_opt, const int32_t* d_n_frames, const int32_t* d_n_seq,
                   int32_t batch, int32_t max_frames, int32_t max_seq, int32_t n_classes, float* d_log_z, float* d_class_post,
                   float* d_state_post, float* d_occ, void* d_workspace, size_t workspace_bytes, void* stream);

/* Decoding.  "Alignment" asks where the phonemes of a KNOWN sequence lie; decoding reads the sequence itself off the
 * scores: the best path through a loop of all C classes, with a transition score between two segments and a minimum
 * duration of M frames per segment (a phone-loop Viterbi recogniser).  Added without a version bump.
 *
 * Inputs, all on the device: d_score [batch, max_frames, C] float32 (log-posteriors or any additive score); d_n_frames
 * int32 [batch], clamped to [0, max_frames]: F; d_trans [C, C] float32, shared by the batch: trans[i, j] is added when a
 * segment of class i ends and one of class j begins (i == j is an ordinary entry: a phoneme said twice); d_init, d_final
 * [C] float32 or NULL (zeros; nothing is added then); min_dur = M in [1, 8]; d_class_map int32 [C] or NULL (the identity),
 * values in [-1, C) as vc_phn_segments takes it.  Every value of score, trans, init and final is finite or -inf; +inf and
 * NaN are OUTSIDE the contract (with them -inf - -inf could form).  Within it no output is NaN except the defined fill.
 *
 *   States      (c, d), d = 0 .. M-1: class c in its (d+1)-th frame, or a later one when d = M-1.  e(t, c) = score[b, t, c].
 *   Recurrence  float32; every operation is one IEEE addition or a strict compare-select; nothing is multiplied.
 *               D(0, (c, 0)) = init[c] + e(0, c) (without init: e(0, c)); D(0, (c, d > 0)) = -inf.
 *               X(t, c) = the maximum over i, taken in ascending order, of D(t-1, (i, M-1)) + trans[i, c], each term rounded
 *               to float32 before the compare; a later i replaces the holder only when strictly greater, so the lowest i
 *               wins a tie; bp(t, c) is that i.
 *               M = 1:  D(t, (c, 0)) = e(t, c) + best; best starts as D(t-1, (c, 0)) (stay) and is replaced by X(t, c)
 *                       (enter) iff that is strictly greater.
 *               M > 1:  D(t, (c, 0)) = e(t, c) + X(t, c);  D(t, (c, d)) = e(t, c) + D(t-1, (c, d-1)) for 0 < d < M-1;
 *                       D(t, (c, M-1)) = e(t, c) + best; best starts as D(t-1, (c, M-1)) (stay) and is replaced by
 *                       D(t-1, (c, M-2)) (advance) iff that is strictly greater.
 *   End         total = the maximum over c, ascending, of D(F-1, (c, M-1)) + final[c] (without final: the bare value), the
 *               lowest c on a tie: the last segment lasts M frames too.  INFEASIBLE iff F == 0, F < M or total == -inf.
 *   Path        read back from the stay / advance (enter) decisions and bp, from (F-1, (c*, M-1)) to frame 0.
 *
 * Outputs, every element written exactly once per call whatever the memory held (no memset, no atomics):
 *   d_frame_class [batch, max_frames] int32   the raw class of every frame; -1 from F on and when infeasible
 *   d_seg_label, d_seg_start, d_seg_end [batch, max_frames] int32 (end exclusive) and d_n_seg [batch] int32: the layout
 *                                             of vc_phn_segments, -1 from the row's n_seg on.  The decoded segments have
 *                                             their labels mapped through class_map, then equal neighbours merge, then
 *                                             segments labelled -1 are removed ("a b a" with b -> -1 stays two "a")
 *   d_seg_score [batch, max_frames] float32   the emissions e(t, frame_class[t]) of the segment's frames widened to
 *                                             float64, added in frame order, divided by their count, rounded once; NaN
 *                                             from n_seg on
 *   d_total [batch] float32                   -inf when infeasible
 * The device equals the float32 restatement of tests/decode_ref.py bit for bit in every output.
 *
 * Two launches on the caller's stream.  Forward: one workgroup per utterance, a lane per destination class with its M
 * values of D in registers; up to 64 classes one wave with its column of trans in registers and the previous row read
 * from the other lanes, up to 128 classes two waves with trans in LDS and one barrier per frame; the maximum over i in
 * four chains over contiguous quarters, merged in order; emissions fetched four frames ahead with a clamped index; one
 * byte of moves per (frame, class).  Back-track: one wave finds each segment's first frame with a ballot over 64 move
 * bytes, then 256 lanes derive the outputs from the frames' classes.  d_workspace (4-byte aligned):
 *     vc_decode_workspace_bytes = align256(4 batch) + align256(batch * C * ceil(max_frames / 4) * 4)
 * (host arithmetic only; 0 for a shape the launch would refuse; too small: VC_ERR_WORKSPACE).  Limits (VC_ERR_UNSUPPORTED
 * beyond them): C <= 128; 1 <= min_dur <= 8; batch <= 65,535; max_frames <= 16,384; the workspace below 2^31 bytes.
 * A function of its own utterance alone: bit-identical alone, in any batch, from run to run and under graph replay;
 * lengths are read on the device; no allocation and no host wait; arguments are checked before any HIP call. */
size_t vc_decode_workspace_bytes(int32_t batch, int32_t max_frames, int32_t n_classes);
int vc_decode_f32(const float* d_score, const int32_t* d_n_frames, const float* d_trans, const float* d_init, const float* d_final,
                  const int32_t* d_class_map, int32_t batch, int32_t max_frames, int32_t n_classes, int32_t min_dur,
                  int32_t* d_frame_class, int32_t* d_seg_label, int32_t* d_seg_start, int32_t* d_seg_end, int32_t* d_n_seg,
                  float* d_seg_score, float* d_total, void* d_workspace, size_t workspace_bytes, void* stream);

/* Duration.  Conversion keeps the source's timing: every output frame sits where its input frame sat.  These two launches
 * move frames in time: an integer time map built from a segment table (as vc_phn_segments, vc_align_f32 and vc_decode_f32
 * write it), and the resampling of a spectrogram along that map, before the vocoder (which rebuilds the phase, so nothing
 * has to stay coherent).  Added without a version bump.  tests/warp_ref.py restates both; the device equals it bit for bit.
 *
 * vc_duration_map.  Inputs, all on the device: d_start, d_end [batch, max_seg] int32 (end exclusive) with d_n_seg [batch],
 * clamped to [0, max_seg]; d_n_frames int32 [batch], clamped to [0, max_frames]: n.  An entry with start < 0 or
 * end == start is ABSENT.  One of: d_out_len [batch, max_seg] int32, the output length of every present segment (>= 0); a
 * rate table d_ratio_q int32 [n_classes], Q16 (65,536 = unchanged), every value clamped to [0, 8 * 65,536] when read, with
 * d_label [batch, max_seg] (values in [0, n_classes)) or, without labels, n_classes == 1 and one rate for every segment;
 * or neither (segments keep their length).  gap_q: the Q16 rate of the frames outside the segments.
 *   Pieces   The present segments must be sorted, must not overlap and must lie in [0, n].  The frames between them,
 *            before the first and from the last one to n are gap pieces.  Piece p has Li input frames from input offset S
 *            and Lo output frames from output offset O (S, O: exclusive prefix sums): Lo = out_len[k], or
 *            (Li * ratio_q[label] + 32768) >> 16 for a segment, (Li * gap_q + 32768) >> 16 for a gap.  Lo == 0 deletes it.
 *   Map      output frame u of piece p, j = u - O:  pos = S * 65536 + ((2j + 1) * Li * 65536) / (2 * Lo) - 32768 (integer
 *            division), clamped to [0, (n - 1) * 65536]: Q16 input frames, the centre-aligned map S + (j + 1/2) Li / Lo - 1/2
 *            to within 2^-16, monotone across pieces, and exactly u * 65536 where every Lo == Li.
 *   Flags    never an error.  1: the table is invalid (unsorted, overlapping, outside [0, n], end < start, a negative
 *            out_len, a label outside the rate table); 2: the total is below min_frames; either way the utterance gets the
 *            IDENTITY map (n frames).  4: the total exceeds out_frames and is cut there.  n == 0: n_out = 0, flags = 0.
 * Outputs, every element written exactly once per call: d_pos [batch, out_frames] int32, -1 from n_out on; d_n_out [batch];
 * d_out_start, d_out_end [batch, max_seg]: the present segments in output frames, clamped to n_out (a deleted segment has
 * an empty range; under flag 2 the input table), -1 for absent entries, from n_seg on, under flag 1 and for n == 0;
 * d_flags [batch].  One workgroup of 1,024 lanes per utterance: the table in tiles of 1,024 entries with the carried state
 * in registers (a running maximum of the ends, a sum scan of the output lengths), then a binary search and one 64-bit
 * division per output frame.  Everything read from the table is range-checked before use and forms no address.
 * d_workspace (8-byte aligned): vc_duration_map_workspace_bytes = align256(batch * (max_seg + 1) * 8) (host arithmetic;
 * 0 for a shape the launch would refuse; too small: VC_ERR_WORKSPACE).  Limits (VC_ERR_UNSUPPORTED beyond them, nothing
 * launched): batch <= 65,535; max_seg, max_frames, out_frames <= 16,384; gap_q in [0, 8 * 65,536].
 *
 * vc_time_warp.  d_src [batch, max_frames, C] float32; d_pos [batch, out_frames] and d_n_out [batch] as above (n_out clamped
 * to [0, out_frames], every pos to [0, (n - 1) * 65536] when read); d_n_frames [batch] or NULL (max_frames), clamped.
 * VC_WARP_LINEAR: with i = pos >> 16, i1 = min(i + 1, n - 1) and w = (pos & 65535) * 2^-16 (exact),
 * dst[u, :] = a + w * (b - a) of rows i and i1 -- three separately rounded float32 operations, no contraction; where w == 0
 * it is row i itself and row i1 is not read.  VC_WARP_NEAREST: row min((pos + 32768) >> 16, n - 1).  Rows from n_out on
 * (all rows when n == 0) are zero.  d_amp [batch, out_frames, C] or NULL: also the vocoder's magnitude of the warped
 * value, exp10(0.05 * (max(0, v) / P_dB_norm_factor - 80)) (vc_compound_stitch's expression, realse == 1), 0 in the zero
 * rows: bit-identical to vc_power_to_amp(dst, n_out).  Streaming: no LDS, no atomics, every destination element written
 * once; 16-byte stores when out_frames * C is a multiple of 4, 16-byte reads when C is.  Limits: batch <= 65,535;
 * max_frames, out_frames <= 16,384; frames * C < 2^30.
 *
 * Both are functions of their own utterance alone, bit-identical alone, in any batch, from run to run and under graph
 * replay; lengths are read on the device; no allocation and no host wait; arguments are checked before any HIP call. */
#define VC_WARP_LINEAR 0
#define VC_WARP_NEAREST 1
size_t vc_duration_map_workspace_bytes(int32_t batch, int32_t max_seg);
int vc_duration_map(const int32_t* d_start, const int32_t* d_end, const int32_t* d_n_seg, const int32_t* d_label,
                    const int32_t* d_out_len, const int32_t* d_ratio_q, int32_t n_classes, int32_t gap_q,
                    const int32_t* d_n_frames, int32_t batch, int32_t max_seg, int32_t max_frames, int32_t min_frames,
                    int32_t out_frames, int32_t* d_pos, int32_t* d_n_out, int32_t* d_out_start, int32_t* d_out_end,
                    int32_t* d_flags, void* d_workspace, size_t workspace_bytes, void* stream);
int vc_time_warp(const float* d_src, const int32_t* d_pos, const int32_t* d_n_out, const int32_t* d_n_frames, int32_t batch,
                 int32_t max_frames, int32_t out_frames, int32_t C, int32_t mode, float* d_dst, float* d_amp,
                 float P_dB_norm_factor, void* stream);

/* Pitch.  Conversion leaves the melody to the decoder and the vocoder; duration conversion moves frames, not harmonics.
 * These two launches change the fundamental of a WAVEFORM and keep its length: overlap-add of two-period grains
 * (time-domain PSOLA) whose positions come from integrating an F0 track -- no search for glottal epochs in the samples:
 * for a periodic signal any placement one period apart is a valid grain sequence.  The plan (marks, grain choice,
 * widths) is integer arithmetic on two tables; the overlap-add is a gather.  Added without a version bump.
 * tests/pitch_ref.py restates both; the device equals it bit for bit.  All plan arithmetic is integer (int64 where noted).
 *
 * Inputs per utterance: x[0, len) float32 samples; len from d_len int32 [batch] (clamped to [0, max_len]), so the output of
 * a launch that keeps its lengths on the device can be fed as it is; hop; n_frames = F frames of two int32 tables,
 * d_period_q[f] and d_ratio_q[f] [batch, F], both Q16: the period of the signal in samples and the factor its fundamental
 * is to be multiplied by.
 *   Clamps   applied when a value is read:  P[f] = clamp(period_q[f], 16 << 16, 1024 << 16);
 *            R[f] = clamp(ratio_q[f], 32768, 131072), a ratio in [0.5, 2];
 *            S[f] = clamp((P[f] * 65536 + R[f] / 2) / R[f], 16 << 16, 2048 << 16), in int64.  No content of either table
 *            gives a step below 16 samples, which bounds every loop.
 *   Frames   fr(m) = min((m + hop / 2) / hop, F - 1): the front-end's centred frames.
 *   Marks    of a step table T:  pos_0 = 0 (int64, Q16), m_k = pos_k >> 16, pos_{k+1} = pos_k + T[fr(m_k)]; the list ends
 *            before the first m_k >= len.  Analysis marks a_0 .. a_{K-1}: T = P; synthesis marks s_0 .. s_{J-1}: T = S.
 *            K, J <= len / 16 + 1.  The step is constant inside a frame, so an implementation may recur over frames and
 *            expand the marks in parallel: frame f ends at Q16 position ((f + 1) * hop - hop / 2) << 16 (the last frame
 *            and every frame cut by len: at len << 16), and the count in a frame is one ceiling division.
 *   Grain j  k(j): the analysis mark nearest to s_j, the lower k of two equally near ones; src_j = a_k(j);
 *            h_j = (P[fr(src_j)] + 32768) >> 16, in [16, 1024].
 *   Window   one table W[i] = float32(0.5 + 0.5 cos(pi i / 2048)), i = 0 .. 2048, made on the host in float64, W[2048] = 0
 *            (d_window, 2,049 floats on the device).  w_j(d) = W[(|d| * 2048 + h_j / 2) / h_j] for |d| < h_j; else grain
 *            j does not cover the sample.
 *   Output   for n < len:  N = sum_j x~[src_j + n - s_j] * w_j(n - s_j),  D = sum_j w_j(n - s_j)  over the covering
 *            grains in ascending j, float32, every product and every sum rounded separately (no contraction), both sums
 *            from +0; x~ is zero outside [0, len).  y[n] = N / max(D, w_floor) (IEEE division); y[n] = 0 for n >= len.
 *            len samples in, len out.  A sample no grain covers is 0 / w_floor = 0.
 *
 * vc_psola_plan writes, per utterance and with M = vc_psola_max_marks(max_len) = max_len / 16 + 1: d_n_a = K, d_n_s = J
 * [batch]; d_a, d_s, d_src, d_h [batch, M] int32, -1 from K (d_a) or J (the others) on; every element exactly once.  One
 * workgroup per utterance: the tables pass through LDS in tiles of 1,024 frames, one lane per mark list walks the tile
 * (one division per frame that holds a mark), all lanes expand the marks; the nearest-mark search is a binary search of at
 * most 22 steps.  Every loop bound comes from F, max_len and tile sizes; nothing read from a table forms an address.
 *
 * vc_psola_ola_f32: grid (tiles of 1,024 outputs, utterance).  A tile stages the grains that can reach it -- s_j within
 * [tile start - 1023, last sample + 1023], found by binary search, at most 192 -- into LDS once; each lane gathers its
 * samples over that list.  No atomics; every element of d_y [batch, max_len] is written exactly once, the zeros from len on
 * included; d_x [batch, max_len] is not read at or beyond len.  The plan is read defensively: n_s is clamped to [0, M], h to
 * [16, 1024], and a staged grain whose s lies outside the searched range or whose src lies outside [0, len) covers nothing.
 * d_y must not be d_x.  w_floor > 0.
 *
 * Both are functions of their own utterance alone, bit-identical alone, in any batch, from run to run and under graph
 * replay; they take everything from device memory, allocate nothing and wait for nothing.  Limits (VC_ERR_UNSUPPORTED
 * beyond them, nothing launched): batch <= 65,535; max_len <= 2^24; n_frames <= 2^20; hop in [1, 65,536]. */
int32_t vc_psola_max_marks(int32_t max_len);
int vc_psola_plan(const int32_t* d_period_q, const int32_t* d_ratio_q, const int32_t* d_len, int32_t batch, int32_t max_len,
                  int32_t n_frames, int32_t hop, int32_t* d_n_a, int32_t* d_n_s, int32_t* d_a, int32_t* d_s, int32_t* d_src,
                  int32_t* d_h, void* stream);
int vc_psola_ola_f32(const float* d_x, const int32_t* d_len, const int32_t* d_n_s, const int32_t* d_s, const int32_t* d_src,
                     const int32_t* d_h, const float* d_window, int32_t batch, int32_t max_len, float w_floor, float* d_y,
                     void* stream);

/* Time scale.  Duration conversion warps SPECTRA along vc_duration_map's time map and leaves the phase to the vocoder.
 * These two launches move a WAVEFORM along the same map: waveform-similarity overlap-add (WSOLA, Verhelst & Roelands).
 * Grains of 2 S samples are copied from the input, one every S output samples; each is chosen within +-tol samples of
 * where the map points so that it continues its predecessor's waveform.  No F0 track is needed, and the local phase of a
 * natural recording survives -- what the differential route (below) needs to change its timing.  Added without a version
 * bump.  tests/wsola_ref.py restates both; every decision is integer arithmetic and the device equals it bit for bit.
 *
 * Inputs per utterance: x[0, len) float32 in a row of d_x [batch, x_stride]; len from d_len int32 [batch], clamped to
 * [0, max_len]; pos[0, n_out) int32 Q16 input frames in a row of d_pos [batch, out_frames] exactly as vc_duration_map
 * writes them, n_out from d_n_out [batch], clamped to [0, out_frames]; every pos is clamped to >= 0 when read and the -1
 * padding from n_out on is never read.  Scalars: hop (samples per frame), group g >= 1, S = g * hop (the synthesis hop),
 * tol >= 0 (the search half width in samples), qscale (float32 > 0).
 *   Sizes      out_len = hop * (n_out - 1) when n_out >= 2 and len >= 1, else 0;
 *              K = ceil(out_len / S) + 1 when out_len > 0, else 0.
 *   Quantised  q[n] = clamp(rint(float32(x[n] * qscale)), -32767, 32767) as an integer: the product rounded once to
 *              float32, then to the nearest integer with ties to even; NaN gives 0, +-inf +-32767.  q~ and x~ are q and x
 *              extended by zeros outside [0, len).
 *   Targets    u_k = min(k * g, n_out - 1);  tau_k = clamp((int64(pos[u_k]) * hop + 32768) >> 16, 0, len - 1): frame u is
 *              centred on sample u * hop, the front-end's convention.
 *   Recurrence a_0 = tau_0, cost_0 = 0.  For k >= 1 with n_k = a_{k-1} + S (the natural continuation) and every d in
 *              [-tol, tol]:  cost(d) = sum_{i = -S}^{S - 1} | q~[tau_k + d + i] - q~[n_k + i] |, exact in int32
 *              (65534 * 2048 < 2^31).  The d of the smallest (cost, |d|, d) in lexicographic order is taken:
 *              a_k = tau_k + d, cost_k = cost(d).  |a_k - tau_k| <= tol always: the chain cannot drift from the map.
 *   Output     for m in [0, out_len): k = m / S, r = m - k * S, A = x~[a_k + r], B = x~[a_{k+1} + r - S],
 *              y[m] = A + T[r] * (B - A) as three separately rounded float32 operations (no contraction);
 *              T[r] = float32(0.5 - 0.5 cos(pi r / S)), r in [0, S), made on the host in float64 (d_window, S floats on the
 *              device).  y is zero from out_len to the row's end, hop * (out_frames - 1).
 * Consequences: where a grain is the natural continuation of its predecessor, A == B and y copies x bit for bit; with the
 * identity map d = 0 costs 0 and wins every tie, so y == x[:out_len]; a signal of integer period P <= 2 tol + 1 always has
 * a candidate of cost 0 while grains and candidates stay inside [0, len), so y[m] == x[(m + a_0) mod P] at any rate.
 *
 * vc_wsola_plan writes, per utterance and with M = vc_wsola_max_grains(out_frames, hop, group) =
 * ceil(hop * (out_frames - 1) / S) + 1 (a host-only query; 0 beyond the limits): d_a [batch, M] int32, INT32_MIN from K on;
 * d_cost [batch, M] int32, -1 from K on; d_n_grains = K and d_out_len [batch]; every element exactly once.  One workgroup of
 * 512 lanes per utterance (the chain over k is sequential): per step the 2 S reference samples and the 2 S + 2 tol samples of
 * the candidate span go into LDS as biased 16-bit integers, two to a dword; candidates go in pairs (2 p, 2 p + 1) that share their dwords, up to 8 lanes share a pair's window, and
 * the 64-bit key (cost, |d|, d) is reduced over the wave by shuffles and over the waves through LDS.
 *
 * vc_wsola_ola_f32: grid (tiles of 1,024 outputs, utterance).  d_y [batch, hop * (out_frames - 1)], every element written
 * exactly once, the zeros from out_len on included (a row of no samples -- out_frames == 1 -- launches nothing); d_x is not
 * read at or beyond len.  The plan is read defensively: d_n_grains is clamped to [0, M], d_out_len to the row, a grain at or
 * beyond the count or with a outside [-2^24, 2^24] covers nothing (its samples count as 0), and no plan value forms an
 * address unchecked.  d_y must not be d_x.
 *
 * Both are functions of their own utterance alone, bit-identical alone, in any batch, from run to run and under graph
 * replay; they take everything from device memory, allocate nothing and wait for nothing.  VC_ERR_INVALID before any HIP
 * call for a NULL pointer, a size below 1, tol < 0, x_stride < max_len or a qscale that is not positive and finite.  Limits
 * (VC_ERR_UNSUPPORTED beyond them, nothing launched): batch <= 65,535; max_len <= 2^24; out_frames <= 16,384; hop in
 * [1, 1024]; S in [1, 1024]; tol in [0, 1024]. */
int32_t vc_wsola_max_grains(int32_t out_frames, int32_t hop, int32_t group);
int vc_wsola_plan(const float* d_x, int32_t x_stride, const int32_t* d_len, const int32_t* d_pos, const int32_t* d_n_out,
                  int32_t batch, int32_t max_len, int32_t out_frames, int32_t hop, int32_t group, int32_t tol, float qscale,
                  int32_t* d_a, int32_t* d_cost, int32_t* d_n_grains, int32_t* d_out_len, void* stream);
int vc_wsola_ola_f32(const float* d_x, int32_t x_stride, const int32_t* d_len, const int32_t* d_a, const int32_t* d_n_grains,
                     const int32_t* d_out_len, const float* d_window, int32_t batch, int32_t max_len, int32_t out_frames,
                     int32_t hop, int32_t group, float* d_y, void* stream);

/* Differential-spectrum conversion (Kobayashi & Toda; sprocket's DIFFVC).  The other conversion entry points SYNTHESISE the
 * converted spectrum with Griffin-Lim.  These two launches FILTER the source recording by the difference between the
 * converted and the source spectral envelope instead: excitation and phase stay the source's own, and the cost is one
 * STFT / ISTFT pass.  Added without a version bump.  tests/diff_ref.py restates both in float64 and the gain in float32.
 *
 * Gain.  d_pred, d_true [batch, max_frames, n_bins] float32: the front-end's normalised power dB (stft_pred, stft_true of
 * conversion.convert_batch).  For every frame f < n_frames[b] (clamped to [0, max_frames]; NULL: all) and bin k:
 *     d[k]  = (max(pred, 0) - max(tru, 0)) / P_dB_norm_factor                 IEEE float32 division
 *     s0[k] = sum_{j = -h .. h} c[j] * d[refl(k + j)]                         h = (n_taps - 1) / 2
 *             c = d_taps, float32 [n_taps] from the caller (symmetric by convention), n_taps odd, <= 65; refl mirrors about
 *             bin 0 and about bin n_bins - 1 without repeating the edge (as often as it takes: n_bins may be smaller than
 *             h); the sum starts from +0 and ascends in j; every product and every sum is rounded once (no fused
 *             multiply-add)
 *     s[k]  = min(max(alpha * s0[k], -max_cut_db), max_boost_db)              a power ratio in dB
 *     G[k]  = exp2f(s[k] * float32(log2(10) / 20))                            an amplitude ratio
 * Rows at or beyond n_frames[b] are written as 0; every element of d_gain [batch, max_frames, n_bins] is written exactly
 * once.  One launch: a workgroup takes a tile of 16 frames, puts each frame's n_bins differences into LDS once with the
 * mirrored edges folded into the index, and every lane then takes bins.  The rows (201 floats) do not start on 16-byte
 * boundaries: they are read element by element, and the flat output slab is stored 16 bytes per lane where its length and
 * address allow.  VC_ERR_INVALID before the launch for a NULL pointer, batch outside [1, 65535], max_frames < 1,
 * n_bins outside [2, 2049], n_taps even or outside [1, 65], a non-finite float, P_dB_norm_factor == 0, alpha outside [0, 1]
 * or a negative clamp.
 *
 * Filter.  With the plan's padded window w, N = n_fft, hop, and per utterance len = d_len[b] clamped to [0, wav_stride] and
 * F_b = min(n_frames[b], max_frames, 1 + len / hop) (d_n_frames NULL: without the first), a negative count counting as 0:
 *     y_b = istft(G_b[f] * stft(x_b)[f], f < F_b)        in librosa's sense (center=True, reflect padding)
 *   input    x_b[0, len) of d_wav [batch, wav_stride], reflect-padded by N / 2 about sample 0 and about sample len - 1: the
 *            signal's own end, not hop * (F_b - 1).  Nothing at or beyond min(len, wav_stride) is read.
 *   synthesis  synthesis window, overlap-add divided by the window sum-square, trimmed by N / 2: what the Griffin-Lim
 *            iteration kernel and its overlap-add kernel do
 *   output   hop * (F_b - 1) samples, then zeros up to out_stride; every element of d_out [batch, out_stride] is written once
 *   short    len <= N / 2 or hop * (F_b - 1) <= N / 2 gives a row of zeros; no length forms an address outside the buffers,
 *            and the lengths are read on the device
 * d_gain [batch, max_frames, n_bins] with n_bins = 1 + N / 2, real: the filter is zero-phase.  n_fft is NOT zero-padded, so
 * the product G * Z is a CIRCULAR convolution within a frame: a gain whose impulse response is longer than the window's
 * taper wraps around the frame's ends, damped only by the synthesis window.  This is not removed; a smooth gain (the taps
 * above) keeps its response short.
 * Workspace (vc_stft_filter_workspace_bytes; 0 for a NULL plan, batch <= 0 or max_frames <= 0; 4-byte aligned): one frame
 * buffer [batch, max_frames, N] float32 rounded up to 256 bytes, whose rows at or beyond F_b are not written, then
 * align256(4 * batch) bytes -- 256 up to 64 utterances -- in which the filter kernel leaves F_b [batch] int32 (0 for a
 * zero row): the overlap-add kernel takes its frame counts from there, since F_b depends on lengths only the device knows.
 * Two launches: the filter kernel (16 frames per workgroup at n_fft == 400, 4 otherwise; gather of the padded waveform,
 * forward transform, G * Z in registers, inverse transform, window), then the vocoder's overlap-add kernel.  VC_ERR_INVALID
 * before any launch for a NULL pointer (d_n_frames excepted), batch outside [1, 65535], max_frames < 1, wav_stride < 1 or
 * out_stride < hop * (max_frames - 1); VC_ERR_WORKSPACE for a workspace that is too small.
 *
 * Neither call allocates, sets memory, uses atomics or synchronises; both are capturable from the first call, functions of
 * their own utterance alone and bit-identical alone, in any batch and under graph replay. */
int vc_spectral_diff_gain_f32(const float* d_pred, const float* d_true, const int32_t* d_n_frames, int32_t batch,
                              int32_t max_frames, int32_t n_bins, float P_dB_norm_factor, float alpha, float max_boost_db,
                              float max_cut_db, const float* d_taps, int32_t n_taps, float* d_gain, void* stream);
size_t vc_stft_filter_workspace_bytes(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames);
int vc_stft_filter_f32(const vc_vocoder_plan* plan, const float* d_wav, int32_t wav_stride, const int32_t* d_len,
                       const float* d_gain, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float* d_out,
                       int32_t out_stride, void* d_workspace, size_t workspace_bytes, void* stream);

/* Postfilters.  A decoder trained on a squared error predicts trajectories -- one spectral bin followed along time -- with
 * too little variance, most of all at the fast modulation frequencies: the muffled sound that realse patches with a power
 * law.  These four launches restore the statistics of natural trajectories: Toda's global-variance (GV) filter and
 * Takamichi's modulation-spectrum (MS) filter, which generalises it.  Added without a version bump.
 * tests/postfilter_ref.py restates all four in float64 and in float32.
 *
 * Data.  d_x [batch, max_frames, channels] float32, channels contiguous: stft_pred, mel_pred or any dB-linear feature.
 * n = d_n_frames[b] (int32 [batch] on the device; NULL: max_frames), clamped to [0, max_frames] when read.  Output rows at or
 * beyond n are written as 0.  Constants: segment length 64 frames, hop 32, 33 modulation bins; window
 * w[t] = float32(0.5 - 0.5 cos(2 pi t / 64)), the periodic Hann window, whose half-overlapped copies sum to 1;
 * tiny = 2^-40; floor = 1e-20 (float32).  Unless said otherwise every operation below is one float32 operation rounded once.
 *
 * vc_traj_stats_f32 -> d_stats [batch, channels, 2] = (mean, population variance) over f < n, both 0 when n == 0:
 *     r = x[0];  mean = r + (sum_f (x[f] - r)) / n;  var = (sum_f (x[f] - mean)^2) / n
 *   so a constant channel has mean == its value and var == 0 exactly.  Order of both sums: the frames f = w, w + 8, w + 16, ...
 *   are added in ascending f for each w in 0 .. 7, starting from 0; then the eight partial sums are added in ascending w.
 *   Grid (channel tiles of 64, utterance), two passes over the utterance; a function of the utterance alone.
 *
 * vc_gv_filter_f32.  With var, mean from d_stats and the target d_gv_t [channels]:
 *     g = 1 + alpha * (sqrt(gv_t[c] / var) - 1), clamped to [1 / g_max, g_max]
 *     g = 1 where var <= tiny, where gv_t[c] <= 0 (or NaN) or where the quotient overflows
 *     d = (g - 1) * (x - mean);  y = x + d, and y = x where d == 0 (so that -0 stays -0)
 *   The product and the sum are not contracted.  alpha = 0 returns x bit for bit.
 *
 * vc_ms_stats_f32 -> d_ms [batch, channels, 33, 3] = (count, sum s, sum s^2) per modulation bin m = 0 .. 32:
 *     segment j = 0 .. ceil(n / 32) covers frames [32 j - 32, 32 j + 32); a frame outside [0, n) takes the value of the
 *     nearest frame inside (edge hold);  v[t] = w[t] * (x[.] - mean),  X_j = DFT64(v), bins 0 .. 32
 *     p = Re^2 + Im^2;  where floor < p <= FLT_MAX:  s = logf(p), count += 1, sum += s, sum2 += s * s
 *   Order: the segments j = w, w + 4, ... in ascending j for each w in 0 .. 3, then the four partial sums in ascending w.
 *   n == 0 gives zeros.  mean is READ from d_stats (the variance there is not used).  The transform's own order of operations
 *   (csrc/pf_dft64.h) is not part of the definition; the tests bound it.
 *
 * vc_ms_filter_f32.  d_coef [channels, 33, 2] = (a, b) and the clamps lo <= 0 <= hi, natural-log amplitude exponents:
 *     g_0 = 1;  for m >= 1: g_m = expf(min(max(a * s + b, lo), hi)) with s as above, and g_m = 1 where p is not above the floor
 *     c_j = iDFT64((g - 1) X_j)                                      (with the 1 / 64)
 *     d = c_early[f] + c_late[f]: the two segments that cover frame f, j = f / 32 and j + 1, the earlier one first
 *     y = x + d, and y = x where d == 0
 *   The correction is additive, so a table of zeros (exp(0) - 1 == 0) returns x bit for bit whatever the transforms round to.
 *   Grid (tiles of 32 frames, channel tiles of 64, utterance): a workgroup computes both segments that cover its 32 frames,
 *   so every segment is transformed twice and nothing is exchanged between workgroups.  One logf and one expf per bin and
 *   segment.  The gain is real and the transform is NOT zero-padded, so the modification is CIRCULAR within a segment: what a
 *   gain's impulse response pushes past one end of the 64 frames comes back at the other.  The analysis window tapers the
 *   input to 0 there, which damps the effect but does not remove it; gains that vary smoothly over m keep the response short.
 *
 * All four: every output element is written exactly once; no atomics, no allocation, no memset, no host wait; capturable in a
 * graph from the first call; functions of their own utterance alone, bit-identical alone, in any batch, under any max_frames
 * and under replay.  VC_ERR_INVALID before any HIP call, outputs untouched, for a NULL pointer (d_n_frames excepted), a size
 * below 1, alpha outside [0, 1], g_max below 1, a non-finite scalar, lo > 0, hi < 0, or d_y == d_x.  Limits
 * (VC_ERR_UNSUPPORTED beyond them, nothing launched): batch <= 65,535, max_frames <= 16,384, channels <= 2,049. */
int vc_traj_stats_f32(const float* d_x, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t channels,
                      float* d_stats, void* stream);
int vc_gv_filter_f32(const float* d_x, const int32_t* d_n_frames, const float* d_stats, const float* d_gv_t, int32_t batch,
                     int32_t max_frames, int32_t channels, float alpha, float g_max, float* d_y, void* stream);
int vc_ms_stats_f32(const float* d_x, const int32_t* d_n_frames, const float* d_stats, int32_t batch, int32_t max_frames,
                    int32_t channels, float* d_ms, void* stream);
int vc_ms_filter_f32(const float* d_x, const int32_t* d_n_frames, const float* d_stats, const float* d_coef, int32_t batch,
                     int32_t max_frames, int32_t channels, float lo, float hi, float* d_y, void* stream);

/* Harmonic-plus-noise vocoder (the STRAIGHT / WORLD / HNM family).  The Griffin-Lim route invents a phase for a magnitude; the
 * differential route keeps the source's excitation.  These five launches WRITE the waveform from a spectral envelope and an
 * F0 contour in one pass: harmonics of the asked-for pitch with minimum-phase phases where a frame is voiced, envelope-shaped
 * noise where it is not and above a voiced cutoff.  Added without a version bump.  tests/hnm_ref.py restates all five: the
 * integers exactly, the rest in float64 with a float32 error model.  n = d_n_frames[b] (NULL: max_frames) is clamped to
 * [0, max_frames] when read; F = max_frames, N = n_fft, nb = 1 + N / 2.
 *
 * vc_env_cepstral_f32.  d_amp [batch, F, nb] float32 linear magnitudes (vc_power_to_amp's, vc_compound_stitch's);
 * d_table float32 [N, 2] = (cos, sin)(2 pi m / N), made by the caller in float64 and indexed by (n k) mod N in integers;
 * order L, 1 <= L < N / 2; iters >= 0; floor > 0.  Per frame f < n:
 *     a_k = logf(max(amp_k, floor))                  (a NaN magnitude counts as floor);      A = a
 *     iters + 1 times:
 *       c_n = (A_0 + (-1)^n A_{N/2} + 2 sum_{k = 1}^{N/2 - 1} A_k cos(2 pi n k / N)) / N      n = 0 .. L
 *       E_k = c_0 + 2 sum_{n = 1}^{L} c_n cos(2 pi n k / N)
 *       on all but the last pass A_k = max(a_k, E_k)                                   (Roebel & Rodet's true envelope)
 *     env_log = E and theta_k = -2 sum_{n = 1}^{L} c_n sin(2 pi n k / N) from the last pass: the minimum phase of exp(E).
 *   Both sums run in ascending index from +0, one fused multiply-add per term, so the only difference from a float64
 *   restatement on the same table is float32 summation (tests/hnm_ref.py bounds it).  Rows f >= n of both outputs are 0.
 *   Grid (tiles of up to 8 frames, utterance): the table, the tile's a and A and its cepstra live in LDS (at most 64 KB; fewer
 *   frames per tile where a long transform needs it, which does not change a value); per pass one lane per (frame, n), a
 *   barrier, one lane per (frame, k), a barrier.  Limits: n_fft <= 2,048, iters <= 1,024.
 *
 * vc_hnm_plan.  d_f0 [batch, F] float32 Hz, 0 = unvoiced (vc_f0_yin_f32's, vc_f0_viterbi_f32's).  All outputs are integers
 * and equal the restatement bit for bit; rows f >= n are 0.
 *     voiced[f] uint8   1 where f0_lo <= f0 <= f0_hi (false for NaN and the infinities)
 *     inc[f]    uint32  the phase advance per sample in units of 2^-32 turn: rint(f0 * float32(2^32 / sr)), the product
 *                       rounded once to float32, ties to even; an unvoiced frame takes the value of the nearest voiced frame
 *                       before it, a leading unvoiced run that of the first voiced frame; 0 everywhere without a voiced frame
 *     slope[f]  int32   floor((inc[f + 1] - inc[f]) / hop) in int64, 0 for f = n - 1
 *     phase[f]  uint32  the phase at sample f hop: the exclusive sum, modulo 2^32, over frames of
 *                       hop inc[f] + slope[f] hop (hop - 1) / 2
 *     flags[b]  int32   bit 0: some f0 != 0 (NaN included) below n was outside the limits and counted as unvoiced
 *   Inside interval f (samples f hop + j, 0 <= j < hop) the phase is phase[f] + j inc[f] + slope[f] j (j - 1) / 2 mod 2^32.
 *   One workgroup of 256 lanes per utterance walks the frames in tiles of 256; the last voiced frame is carried by a maximum
 *   scan and the phase by a wrapping sum scan (addition modulo 2^32 is associative: the parallel scan IS the sequential sum).
 *   0 < f0_lo <= f0_hi <= sr / 2; hop <= 4,096.
 *
 * vc_noise_init_f32.  d_noise [batch, max_len]: noise[i] = float32(sqrt(12)) * (U - 0.5), U = (x >> 8) * 2^-24 (the
 * difference is exact, the product rounded once): unit variance.  x is word i % 4 of the Philox4x32-10 block with counter
 * (i / 4, utt_id, 0, 0) and key (seed low, seed high) -- vc_phase_init's addressing with the sample index for the element, so
 * an utterance's noise depends on (seed, utt_id) alone.  d_utt_id NULL: the row index.  0 from d_lens[b] (clamped to
 * [0, max_len]; NULL: max_len) on.
 *
 * vc_hnm_noise_gain_f32.  d_gain [batch, F, n_bins]: gscale * exp2f(env_log * float32(log2 e)) in unvoiced frames (all bins)
 * and, in voiced frames, for bins >= cutoff_bin; 0 below cutoff_bin in voiced frames and for f >= n.  With
 * gscale = noise_level / sqrt(sum w^2) of the vocoder plan's window, vc_stft_filter_f32 applied to the unit-variance noise
 * with this gain gives noise of the envelope's magnitude in expectation (E |STFT|^2 = sum w^2 for white noise).
 *
 * vc_hnm_synth_f32.  d_y [batch, hop (F - 1)].  Interval f < n - 1 has the ends e in {f, f + 1}.  With
 * K_e = min(256, (cutoff_inc - 1) / inc[e]) where voiced[e] and inc[e] > 0, else 0 -- harmonic k is ALIVE at end e when
 * k inc[e] < cutoff_inc, and at most vc_hnm_max_harmonics() = 256 are -- the interval evaluates k = 1 .. max(K_f, K_{f+1}):
 *     position  q = k inc[e] N as a 64-bit integer: bin i = q >> 32, fraction r = float32(q mod 2^32) * 2^-32;
 *               lerp(x) = fma(r, x[min(i + 1, nb - 1)] - x[i], x[i])
 *     a_e = scale * exp2f(lerp(env_log[e]) * float32(log2 e)) at a live end, 0 at a dead one;   scale = 2 / sum w
 *     t_e = lerp(theta[e]) at a live end, the other end's at a dead one
 *     u = float32(j) / float32(hop) (IEEE);  a = fma(u, a_{f+1} - a_f, a_f);  t = fma(u, t_{f+1} - t_f, t_f): equal ends give
 *               the end value exactly
 *     x = fma(t, float32(1 / (2 pi)), float32(int32(k phi_j mod 2^32)) * 2^-32)  turns;   phi_j the plan's phase at j
 *     acc = fma(a, cos2pi(x), acc), from +0, k ascending;  cos2pi: x - rint(x) (exact), z = 1/4 - |x|, z P(z^2) with the
 *               five float32 coefficients of csrc/vc_hnm.hip (3.1e-8 from sin(2 pi z) before rounding)
 *     y = acc, or with d_add: acc + add where a harmonic was evaluated and add itself where none was.
 *   Onsets, offsets and harmonics that cross the cutoff so fade over one hop.  Samples from hop (n - 1) on are 0.
 *   Grid (tiles of vc_hnm_tile_intervals() = 16 intervals, utterance): a tile writes (a_e[k], t_e[k]) for its 17 frames into
 *   LDS -- the exponentials are per frame -- then every lane takes samples 256 apart and loops over k.  cutoff_inc in
 *   [1, 2^31]; hop <= 4,096; n_fft <= 2,048; d_add must not be d_y.
 *
 * All five: every output element is written exactly once; no atomics, no allocation, no memset, no host wait; capturable in a
 * graph from the first call; functions of their own utterance alone, bit-identical alone, in any batch and under replay.
 * VC_ERR_INVALID before any HIP call for a NULL pointer (d_n_frames, d_lens, d_utt_id, d_add excepted), a size below 1 or a
 * scalar outside what is said above.  Limits (VC_ERR_UNSUPPORTED beyond them, nothing launched): batch <= 65,535,
 * max_frames <= 16,384, and those named with each call. */
int32_t vc_hnm_max_harmonics(void);
int32_t vc_hnm_tile_intervals(void);
int vc_env_cepstral_f32(const float* d_amp, const int32_t* d_n_frames, const float* d_table, int32_t batch, int32_t max_frames,
                        int32_t n_fft, int32_t order, int32_t iters, float floor, float* d_env_log, float* d_theta,
                        void* stream);
int vc_hnm_plan(const float* d_f0, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t sr, int32_t hop,
                float f0_lo, float f0_hi, uint8_t* d_voiced, uint32_t* d_inc, int32_t* d_slope, uint32_t* d_phase,
                int32_t* d_flags, void* stream);
int vc_noise_init_f32(const int32_t* d_lens, const int32_t* d_utt_id, int32_t batch, int32_t max_len, int64_t seed,
                      float* d_noise, void* stream);
int vc_hnm_noise_gain_f32(const float* d_env_log, const uint8_t* d_voiced, const int32_t* d_n_frames, int32_t batch,
                          int32_t max_frames, int32_t n_bins, int32_t cutoff_bin, float gscale, float* d_gain, void* stream);
int vc_hnm_synth_f32(const float* d_env_log, const float* d_theta, const uint8_t* d_voiced, const uint32_t* d_inc,
                     const int32_t* d_slope, const uint32_t* d_phase, const int32_t* d_n_frames, const float* d_add,
                     int32_t batch, int32_t max_frames, int32_t n_fft, int32_t hop, int64_t cutoff_inc, float scale, float* d_y,
                     void* stream);

/* Noise suppression.  Every conversion route assumes a clean recording; these two launches, with vc_stft_filter_f32 behind
 * them, take stationary noise out of a waveform first: linear short-time power, then a noise tracker and a suppression
 * gain in one scan over time, then the filter.  Added without a version bump.  tests/denoise_ref.py restates both in float64
 * and, in the operation order below, in float32.
 *
 * Power.  P[b, f, k] = |stft(x_b)[f, k]|^2 with exactly the framing of vc_stft_filter_f32 above: the plan's padded window,
 * reflect padding by N / 2 about sample 0 and about sample len - 1 (len = d_len[b] clamped to [0, wav_stride]),
 * F_b = min(n_frames[b], max_frames, 1 + len / hop) (d_n_frames NULL: without the first; a negative count counts as 0), and
 * the "short" rule: len <= N / 2 or hop * (F_b - 1) <= N / 2 gives F_b = 0.  d_power [batch, max_frames, 1 + N / 2] float32:
 * every element is written once, rows at or beyond F_b as 0.  d_frames_out [batch] int32 receives F_b, so the launches
 * behind this one read it on the device and the host never learns it.  One launch, no workspace: 16 frames per workgroup
 * and the 25 x 16 transform at n_fft == 400, 4 frames and the direct transform otherwise (the forward halves of the filter
 * kernels).  VC_ERR_INVALID before the launch for a NULL pointer (d_n_frames excepted), batch outside [1, 65535],
 * max_frames < 1 or wav_stride < 1.
 *
 * Gain.  d_power [batch, max_frames, n_bins]; F = d_n_frames[b] clamped to [0, max_frames] (NULL: max_frames); d_noise0
 * [batch, n_bins] or NULL: the noise power to start from.  The tracker is Gerkmann & Hendriks (2012): the speech-presence
 * probability under a FIXED prior SNR xi_h1 weighs the periodogram against the running estimate; it is continuous in its
 * input apart from the 0.99 guard.  The rule is Wiener (rule 0) or Ephraim & Malah's log-MMSE (rule 1) on the
 * decision-directed a-priori SNR with Cappe's lower limit xi_min.  float32 throughout, no fused multiply-add, IEEE
 * division; every product and every sum is rounded once.  Per (b, k), y = P[b, f, k]:
 *     k1 = 1 + xi_h1;  c1 = xi_h1 / k1;  q_spp = 1 - a_spp;  q_n = 1 - a_noise;  q_dd = 1 - a_dd
 *     n0 = min(n_init, F)
 *     s  = noise0[b, k] if given, else (sum_{f < n0} P[f, k], ascending from +0) / float(n0);   s = max(s, FLT_MIN)
 *     pb = 0.5
 *     for f in 0 .. F - 1:
 *         t  = min((y / s) * c1, 80)
 *         p  = 1 / (1 + k1 * exp(-t))
 *         pb = a_spp * pb + q_spp * p
 *         if pb > 0.99f: p = min(p, 0.99f)
 *         e  = (1 - p) * y + p * s
 *         s  = max(a_noise * s + q_n * e, FLT_MIN)
 *         g  = min(y / s, gamma_max)
 *         r  = 1 if f == 0 else min(A / s, gamma_max)
 *         xi = max(a_dd * r + q_dd * max(g - 1, 0), xi_min)
 *         w  = xi / (1 + xi)
 *         G  = w                                             rule 0
 *         G  = w * exp(0.5 * E1(max(w * g, 1e-6f)))          rule 1
 *         G  = min(max(G, gain_min), 1);   A = (G * G) * y
 *         gain[f, k] = G;  noise[f, k] = s
 * E1 in Horner form, Abramowitz & Stegun: on x <= 1 (5.1.53)  (((((a5 x + a4) x + a3) x + a2) x + a1) x + a0) - ln x  with
 * a0 .. a5 = -0.57721566, 0.99999193, -0.24991055, 0.05519968, -0.00976004, 0.00107857; on x > 1 (5.1.56)
 * (exp(-x) / x) * (n / d), n = (((x + 8.5733287401) x + 18.0590169730) x + 8.6347608925) x + 0.2677737343,
 * d = (((x + 9.5733223454) x + 25.6329561486) x + 21.0996530827) x + 3.9584969228.
 * Hence: a_noise == 1 freezes s bit for bit; scaling P and noise0 by 2^m scales noise by exactly 2^m and leaves gain
 * bit-identical (away from FLT_MIN and overflow); rule 0 with a_dd == 0, a_noise == 1 and noise0 given involves no
 * transcendental and is reproducible bit for bit.
 * d_gain and (optional) d_noise [batch, max_frames, n_bins]: every element written exactly once, rows at or beyond F as 0.
 * One launch, grid (64-bin groups, batch), one lane per (utterance, bin) walking time with the next frames of P prefetched
 * into registers: latency-bound by design.  VC_ERR_INVALID before the launch for NULL d_power, d_gain or cfg, batch outside
 * [1, 65535], max_frames < 1, n_bins outside [2, 2049], rule not 0 or 1, n_init < 1, a_spp or a_dd outside [0, 1], a_noise
 * outside (0, 1], a non-finite or non-positive xi_h1, xi_min or gamma_max, gain_min outside (0, 1].
 *
 * Neither call allocates, sets memory, uses atomics or synchronises; both are capturable from the first call, functions of
 * their own utterance alone and bit-identical alone, in any batch and under graph replay. */
typedef struct vc_denoise_cfg {
    int32_t rule;       /* 0: Wiener, 1: log-MMSE */
    int32_t n_init;     /* frames averaged for the first noise estimate when d_noise0 is NULL */
    float a_spp;        /* smoothing of the speech-presence probability */
    float a_noise;      /* smoothing of the noise power */
    float a_dd;         /* decision-directed weight */
    float xi_h1;        /* the tracker's fixed prior SNR (linear) */
    float xi_min;       /* lower limit of the a-priori SNR (linear) */
    float gain_min;     /* gain floor (amplitude) */
    float gamma_max;    /* upper limit of the a-posteriori SNR */
} vc_denoise_cfg;
int vc_stft_power_f32(const vc_vocoder_plan* plan, const float* d_wav, int32_t wav_stride, const int32_t* d_len,
                      const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float* d_power, int32_t* d_frames_out,
                      void* stream);
int vc_noise_gain_f32(const float* d_power, const int32_t* d_n_frames, const float* d_noise0, int32_t batch,
                      int32_t max_frames, int32_t n_bins, const vc_denoise_cfg* cfg, float* d_gain, float* d_noise,
                      void* stream);

/* Intelligibility.  The scores of a TIME-ALIGNED pair, clean reference x against processed signal y (a denoiser's, a
 * resampler's, a filter's output): STOI (Taal, Hendriks, Heusdens & Jensen 2011), ESTOI (Jensen & Taal 2016) and SI-SDR
 * (Le Roux, Wisdom, Erdogan & Hershey 2019).  Added without a version bump.  csrc/vc_stoi.hip; tests/stoi_ref.py restates
 * every stage in float64 and the band and score stages, in the operation order below, in float32.
 *
 * Constants.  The waveforms are at 10 kHz (resample first).  W = 256, H = 128, a 512-point transform, N = 30 frames per
 * segment, clip c = 1 + 10^(15 / 20), eps = 2^-52 (the same float32 constant on both sides).  w = hanning(W + 2)[1 : -1],
 * w[n] = 0.5 - 0.5 cos(2 pi (n + 1) / (W + 1)), computed in float64 on the device and rounded once.
 *
 * Framing (MATLAB's).  A signal of L samples has the frames that start at i H for every i H < L - W: F = ceil((L - W) / H),
 * 0 for L <= W.  L = d_lens[b] clamped to [0, max_len] (NULL: max_len); no sample at or beyond L is read.
 *
 * vc_stoi_energy_f32.  d_energy [batch, max_frames] float32: e[f] = sum_n (x[f H + n] w[n])^2 of the REFERENCE, rows at or
 * beyond F as 0; d_n_frames [batch] int32 receives F.  Lane l of a wave adds n = l, l + 64, l + 128, l + 192 in that order,
 * the 64 partial sums are added in a butterfly.  max_frames must hold ceil((max_len - W) / H) frames and be at most 16,384.
 *
 * vc_stoi_keep_f32.  The frames with e[f] > float32(ratio * max_f e[f]), ratio = 10^(-dyn / 10) in (0, 1), ascending:
 * d_index [batch, max_frames] int32, -1 from K on; d_n_kept [batch] receives K.  An utterance with no frame, or of digital
 * silence (max e = 0), has K = 0: nothing is kept "instead", unlike vc_mask_compact, so silence cannot reach a score.
 * (vc_activity_mask and vc_mask_compact are not used: the first reads one frame of an utterance that has none, the second
 * keeps all frames when none is active.)  One workgroup of 1,024 lanes per utterance: max_frames <= 16,384, 209 s.
 *
 * vc_stoi_bands_f32.  d_T [2, batch, max_m, n_bands] float32, signal 0 the reference and 1 the processed one, both through the
 * REFERENCE's list.  M = max(K - 1, 0) clamped to max_m frames; rows at or beyond M as 0.  Frame m is the frame m of the
 * overlap-add (hop H) of the kept, windowed frames, which is never built:
 *     n <  H:  z[n] = (w[n + H] x[idx[m - 1] H + H + n]  +  w[n] x[idx[m] H + n]) w[n]      (m = 0: the second product alone)
 *     n >= H:  z[n] = (w[n] x[idx[m] H + n]  +  w[n - H] x[idx[m + 1] H + n - H]) w[n]
 *     X = the 512-point transform of z followed by 256 zeros;  T[m, j] = sqrt(sum_{k = lo_j}^{hi_j - 1} |X[k]|^2), k ascending
 * d_bands [n_bands, 2] int32 holds (lo_j, hi_j), clamped on the device to 0 <= lo <= hi <= 257; n_bands in [1, 32].  An
 * entry of d_index outside [0, (max_len - W) / H] counts as a frame of zeros.  The transform is a radix-2 Stockham
 * autosort, decimation in frequency: stage t = 0 .. 8 has stride s = 2^t and, for j < 256, p = j / s, q = j % s,
 *     out[q + 2 s p] = in[j] + in[j + 256];   out[q + 2 s p + s] = (in[j] - in[j + 256]) tw[p s]
 * with tw[i] = exp(-2 pi i sqrt(-1) / 512) from float64, the complex product as (ar wr - ai wi, ar wi + ai wr), no
 * product at stage 8 (tw[0]), and stage 0 reduced to out[2 j] = z[j], out[2 j + 1] = z[j] tw[j].  float32, no fused
 * multiply-add.  One wave per (signal, utterance, frame), four frames per workgroup, 35 KB of LDS; grid (ceil(max_m / 4),
 * batch, 2).
 *
 * vc_stoi_score_f32.  Two launches.  S = max(M - N + 1, 0) clamped to max_seg segments; segment s is T[s : s + N].
 * mode 0 (STOI), per band j, x and y the N values of the band, all sums ascending from +0:
 *     a = sqrt(sum x^2) / (sqrt(sum y^2) + eps);   y' = min(a y, c x)
 *     mx = (sum x) / N;  my = (sum y') / N;  dx = sqrt(sum (x - mx)^2) + eps;  dy = sqrt(sum (y' - my)^2) + eps
 *     d_j = sum ((x - mx) / dx) ((y' - my) / dy);      seg[s] = (sum_j d_j) / n_bands
 * mode 1 (ESTOI): per band j, mx_j, dx_j, my_j, dy_j as above on x and y themselves; per frame n, xr_j = (x[n, j] - mx_j) /
 * dx_j and yr_j likewise, ax = (sum_j xr_j) / n_bands, ex = sqrt(sum_j (xr_j - ax)^2) + eps, ay and ey likewise,
 *     p_n = sum_j ((xr_j - ax) / ex) ((yr_j - ay) / ey);      seg[s] = (sum_n p_n) / N
 * float32, no fused multiply-add, IEEE division.  d_seg [batch, max_seg]: every element written once, those at or beyond S
 * as 0.  d_score [batch] = float32((sum_{s < S} seg[s] in float64: lane t of 256 adds s = t, t + 256, ..., then a fixed
 * tree) / S); d_n_segments [batch] int32 = S.  S = 0 (too short, or nothing kept) gives score 0: read the count; no NaN is
 * produced.  A band that is zero in y, or in both, contributes d_j = 0.  max_seg <= 16,384.
 *
 * vc_si_sdr_f32.  Over the first L samples, with zero_mean each signal less its own mean:
 *     alpha = <y, x> / <x, x>;   si_sdr = 10 log10(|alpha x|^2 / |alpha x - y|^2),  the residual summed element by element
 * One workgroup of 1,024 lanes per utterance; every sum in float64, lane t adding i = t, t + 1024, ..., then the tree of
 * vc_speech_gain_f32; one rounding to float32 at the end.  L = 0 or <x, x> = 0: si_sdr 0 and valid 0.  A zero residual
 * gives +inf (y == x: the right answer; a multiple of x only where alpha x - y vanishes exactly); alpha = 0 (y orthogonal
 * to x, or zero) gives -inf.
 *
 * None of the five calls allocates, sets memory, uses atomics or synchronises; every output element is written exactly
 * once; all are capturable from the first call, functions of their own utterance alone and bit-identical alone, in any
 * batch and under graph replay.  VC_ERR_INVALID before the launch for a NULL pointer (d_lens excepted), batch outside
 * [1, 65535], max_len outside [1, 2^30], ld < max_len, max_frames, max_m or max_seg outside [1, 16384],
 * max_frames below the frames of max_len (energy), n_bands outside [1, 32], ratio outside (0, 1), mode or zero_mean not
 * 0 or 1. */
int vc_stoi_energy_f32(const float* d_ref, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, float* d_energy,
                       int32_t* d_n_frames, int32_t max_frames, void* stream);
int vc_stoi_keep_f32(const float* d_energy, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float ratio,
                     int32_t* d_index, int32_t* d_n_kept, void* stream);
int vc_stoi_bands_f32(const float* d_ref, const float* d_deg, int32_t batch, int32_t max_len, int32_t ld, const int32_t* d_index,
                      const int32_t* d_n_kept, int32_t max_frames, const int32_t* d_bands, int32_t n_bands, float* d_T, int32_t max_m,
                      void* stream);
int vc_stoi_score_f32(const float* d_T, const int32_t* d_n_kept, int32_t batch, int32_t max_frames, int32_t max_m, int32_t n_bands,
                      int32_t mode, float* d_seg, int32_t max_seg, float* d_score, int32_t* d_n_segments, void* stream);
int vc_si_sdr_f32(const float* d_ref, const float* d_deg, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld,
                  int32_t zero_mean, float* d_si_sdr, uint8_t* d_valid, void* stream);

/* Spectral mapping.  The conversion that needs no encoder and no decoder: a joint-density Gaussian mixture over pairs of
 * source and target feature vectors, fitted by EM along DTW paths of a few parallel sentences, and maximum-likelihood
 * parameter generation (MLPG) of the target's static cepstra from the conditional statistics (Toda, Black and Tokuda
 * 2007).  Added without a version bump.  DESIGN.md section 32; csrc/vc_mapping.hip.
 *
 * Features are vc_spk_features_f32's with deltas = 1, cmn = 0: n cepstra and their regression over +-2 frames, D = 2 n.
 * Limits (VC_ERR_UNSUPPORTED beyond them): 1 <= M <= 256; 1 <= D <= 64; n <= 32; batch <= 65,535; frames * D <= 2^30;
 * max_path <= 2^24; MLPG max_frames <= 2^20.  Lengths are int32 [batch] ON THE DEVICE and clamped to [0, max].
 *
 * The model: d_w [M]; d_mu_x, d_mu_y, d_var_x, d_var_y, d_cov_xy [M, D], float32.  Sxx, Syy and Sxy of a component are
 * diagonal: dimension d of component m carries the 2 x 2 covariance (sxx, sxy; sxy, syy) with det = sxx syy - sxy^2 > 0.
 *
 * vc_jd_prepare_f32 writes the table the other launches read, vc_jd_table_floats(M, D) = 10 M D + 2 M floats.  All of it is
 * float64 arithmetic on the widened parameters WITHOUT contraction, each output rounded once:
 *     [d][m] x 6:  mu_x; mu_y; a = syy / det; b = sxy / det; g = sxx / det; 1 / sxx          (det = sxx * syy - sxy * sxy)
 *     [m]    x 2:  c_m  = log w_m - 0.5 * sum_d log((2 pi)^2 det_md);  cx_m = log w_m - 0.5 * sum_d log(2 pi sxx_md)
 *                  (d ascending from +0; the constants 39.478417604357434 and 6.283185307179586 times det or sxx, then log)
 *     [m][d] x 4:  mu_x; mu_y; A = sxy / sxx; 1 / Dv with Dv = syy - (sxy * sxy) / sxx
 *
 * vc_jd_accumulate_f32: the E-step over the cells of a path.  d_feat_a [batch, max_a, D], d_feat_b [batch, max_b, D];
 * d_path [batch, max_path, 2] int32 with d_path_len [batch] as vc_dtw_backtrack / vc_path_map write them, or both NULL
 * with max_path = 0 for the cells (p, p), p < min(len_a, len_b).  A cell (i, j) with i outside [0, len_a) or j outside
 * [0, len_b) -- (-1, -1) included -- is skipped: nothing is read through it.  Per cell, float32:
 *     l_m = c_m - 0.5 * q,  q = sum_d [ (a dx) dx + ((-2 b) dx) dy + (g dy) dy ],  dx = x_d - mu_x, dy = y_d - mu_y:
 *           d ascending from +0; per d three fused multiply-adds in that order, the first factor of each a rounded
 *           product; then l_m = fma(-0.5, q, c_m)
 *     ll, gamma_m = exp(l_m - ll): as vc_gmm_loglik_f32 / vc_gmm_accumulate_f32
 * Outputs, FLOAT64: d_N [M] = sum gamma; d_S [5, M, D] = the sums of gamma x, gamma y, gamma x^2, gamma y^2, gamma x y
 * (gx = gamma * x rounded; then fma(gx, x, .), fma(gy, y, .), fma(gx, y, .)); d_L [2] = the sum of ll and the number of
 * cells kept.  Nothing of size cells x M or cells x D is stored.  Grid = ceil(M / 64) x 128 partitions: tile k (32 cells)
 * of pair b goes to partition (b + k) mod 128; a partition walks its pairs and tiles ascending, cell by cell; the 128
 * partial sums of an element meet in the order 0 .. 127 in a second launch.  Lane (m, r) of 512 owns component m of the
 * chunk and the dimensions r, r + 8, ...: 40 float64 sums and N in registers.  With M > 64 every chunk forms all M
 * likelihoods of its tiles again (ll needs them).  Workspace: vc_jd_workspace_size(M, D) =
 *     128 * ceil(M / 64) * (64 (1 + 5 D) + 2) * 8 bytes rounded up to 256:
 * independent of the number of frames and of batch; 8-byte aligned; need not be cleared.  VC_ERR_WORKSPACE when too small.
 *
 * vc_jd_update_f32: elementwise, float64 without contraction, each output rounded once.
 *     w_m = max(N_m / sum_k N_k, 2^-40)  (k ascending; not renormalised);  mu = S / N;
 *     var = max(S2 / N - mu * mu, floor[d]) with the unrounded mu (d_floor_x, d_floor_y [D]);
 *     cov = min(max(Sxy / N - mu_x * mu_y, -lim), lim),  lim = rho_max * sqrt(var_x * var_y) of the floored variances.
 * A component with N_m < min_count, or N_m = 0, keeps its means, variances and covariance bit for bit; its weight is
 * still set from N (else the weights would no longer sum to 1).
 *
 * vc_jd_map_f32: conversion statistics per frame of d_feat [batch, max_frames, D].  l_m = cx_m - 0.5 sum_d (x - mu_x)^2 *
 * (1 / sxx) and ll exactly as vc_gmm_loglik_f32; gamma_m = exp(l_m - ll).  With E_md = fma(A, x_d - mu_x, mu_y) and
 * gp = gamma_m * (1 / Dv_md) (one rounded product), m ascending from +0:
 *     P[t, d] = P + gp;   R[t, d] = fma(gp, E, R);   mmse[t, d] = fma(gamma_m, E, mmse)
 * mixture = 0 ("soft") sums over all m; mixture = 1 ("best") takes the one term of the arg-max of l_m (ties to the
 * smallest m) with gamma = 1.  d_best [batch, max_frames] int32 receives the arg-max (required for mixture = 1, else
 * optional); d_mmse may be NULL.  Rows at or beyond the length are 0 in every output.  One workgroup per (utterance, tile
 * of vc_jd_tile() = 32 frames); nothing of size frames x M is stored.
 *
 * vc_mlpg_f32: per utterance and static dimension j < n the trajectory y [F] that minimises
 *     sum_t Ps_t (y_t - Es_t)^2 + Pd_t ((W y)_t - Ed_t)^2,   Ps = P[., j], Pd = P[., n + j], Rs = R[., j], Rd = R[., n + j]
 * (R = P E), W the regression window of vc_spk_features_f32.  With c(t, i) the integer weight of y_i in 10 (W y)_t,
 *     c(t, i) = [i = min(t+1, F-1)] - [i = max(t-1, 0)] + 2 [i = min(t+2, F-1)] - 2 [i = max(t-2, 0)]   in {-3 .. 3},
 *     A[i, k] = Ps_i [i = k] + (sum_t (c(t, i) c(t, k)) Pd_t) / 100,     b_i = Rs_i + (sum_t c(t, i) Rd_t) / 10,
 * both sums over t = max(i-2, 0) .. min(i+2, F-1) ascending from +0, the integer product converted, then multiplied; a term
 * whose integer weight is 0 is left out (nothing is multiplied by 0).
 * A is symmetric positive definite with half-bandwidth 4.  The solve, in FLOAT64 without contraction, IEEE division,
 * for i = 0 .. F-1 ascending (entries with a negative index are 0, their d is 1):
 *     for s = 0 .. 3, k = i-4+s:  v_s = A[i, k] - v_0 L[k, i-4] - ... - v_{s-1} L[k, k-1]   (left to right);
 *                                 L[i, k] = v_s / d_k
 *     d_i = A[i, i] - v_0 L[i, i-4] - v_1 L[i, i-3] - v_2 L[i, i-2] - v_3 L[i, i-1]
 *     z_i = b_i - L[i, i-4] z_{i-4} - L[i, i-3] z_{i-3} - L[i, i-2] z_{i-2} - L[i, i-1] z_{i-1};     u_i = z_i / d_i
 * then for i = F-1 .. 0:  y_i = u_i - L[i+1, i] y_{i+1} - L[i+2, i] y_{i+2} - L[i+3, i] y_{i+3} - L[i+4, i] y_{i+4}
 * (terms beyond F-1 are 0), rounded once to float32.  A pivot d_i that is not positive and finite sets bit 0 of
 * d_flags[b] (written 0 otherwise) and that dimension's whole trajectory becomes Rs_t / Ps_t (float64 quotient, rounded
 * once).  d_y [batch, max_frames, n]; rows at or beyond the length are 0.  One wave per utterance, one lane per
 * dimension; the inputs of a row are loaded three rows ahead of the elimination; the factor goes to the workspace by
 * COLUMNS, [utterance][i][5][n] float64 = L[i+4, i], L[i+3, i], L[i+2, i], L[i+1, i], u_i -- what the back substitution of
 * row i reads, again three rows ahead --, so that a wave's accesses are consecutive.  vc_mlpg_workspace_size(batch, max_frames, n) = batch * max_frames * 5 * n * 8 bytes rounded up to 256.
 *
 * vc_cep_gain_f32: converted static cepstra d_cep_pred and the source's d_cep_src [batch, max_frames, n] to the gain
 * [batch, max_frames, n_bins] of vc_stft_filter_f32.  float32, every product and sum rounded on its own, ascending from +0:
 *     dmel_k = sum_i d_dct[i, k] * (y_i - x_i)            d_dct [n, n_mels]: the rows of the DCT the cepstra were made with
 *     dbin   = (1 - w) * dmel[i0] + w * dmel[i0 + 1]      d_bin_i0 int32 [n_bins] (clamped to [0, n_mels - 2]), d_bin_w [n_bins]
 *     s      = min(max((alpha * db_scale) * dbin, -max_cut_db), max_boost_db);     G = exp2f(s * float32(log2(10) / 20))
 * Rows at or beyond d_n_frames[b] (NULL: none) are 0.  n_mels in [2, 128], n_bins <= 2049.
 *
 * None of the launches allocates, sets memory, uses atomics or synchronises; every output element is written exactly
 * once; all are capturable and bit-identical alone, in any batch and under graph replay (the E-step's sums depend on
 * the batch they are taken over, by definition).  Arguments are checked before any HIP call. */
int vc_jd_tile(void);
size_t vc_jd_table_floats(int32_t M, int32_t D);
size_t vc_jd_workspace_size(int32_t M, int32_t D);
size_t vc_mlpg_workspace_size(int32_t batch, int32_t max_frames, int32_t n_coef);
int vc_jd_prepare_f32(const float* d_w, const float* d_mu_x, const float* d_mu_y, const float* d_var_x, const float* d_var_y,
                      const float* d_cov_xy, int32_t M, int32_t D, float* d_table, void* stream);
int vc_jd_accumulate_f32(const float* d_feat_a, const float* d_feat_b, const int32_t* d_len_a, const int32_t* d_len_b,
                         const int32_t* d_path, const int32_t* d_path_len, int32_t batch, int32_t max_a, int32_t max_b,
                         int32_t max_path, int32_t D, const float* d_table, int32_t M, double* d_N, double* d_S, double* d_L,
                         void* d_workspace, size_t workspace_bytes, void* stream);
int vc_jd_update_f32(const double* d_N, const double* d_S, int32_t M, int32_t D, const float* d_mu_x_in, const float* d_mu_y_in,
                     const float* d_var_x_in, const float* d_var_y_in, const float* d_cov_in, const float* d_floor_x,
                     const float* d_floor_y, float rho_max, float min_count, float* d_w_out, float* d_mu_x_out, float* d_mu_y_out,
                     float* d_var_x_out, float* d_var_y_out, float* d_cov_out, void* stream);
int vc_jd_map_f32(const float* d_feat, const int32_t* d_len, int32_t batch, int32_t max_frames, int32_t D, const float* d_table,
                  int32_t M, int32_t mixture, float* d_P, float* d_R, float* d_mmse, int32_t* d_best, void* stream);
int vc_mlpg_f32(const float* d_P, const float* d_R, const int32_t* d_len, int32_t batch, int32_t max_frames, int32_t n_coef,
                float* d_y, int32_t* d_flags, void* d_workspace, size_t workspace_bytes, void* stream);
int vc_cep_gain_f32(const float* d_cep_pred, const float* d_cep_src, const int32_t* d_n_frames, int32_t batch, int32_t max_frames,
                    int32_t n_coef, const float* d_dct, int32_t n_mels, const int32_t* d_bin_i0, const float* d_bin_w, int32_t n_bins,
                    float alpha, float db_scale, float max_boost_db, float max_cut_db, float* d_gain, void* stream);

/* Dereverberation.  Late reverberation follows the speech, so the noise tracker above cannot take it out.  Weighted
 * prediction error (WPE; Nakatani et al. 2010, in the formulation of Drude et al. 2018, nara_wpe) does: per frequency bin a
 * delayed linear predictor over past STFT frames, estimated by iteratively re-weighted least squares, is subtracted.  It is
 * linear, keeps the phase and needs no training.  Three launches: the complex STFT, the solver, the inverse.  Added
 * without a version bump.  tests/dereverb_ref.py restates all three in float64 numpy, the solver in the order below.
 *
 * vc_stft_complex_f32: Z = stft(x) with exactly the framing of vc_stft_filter_f32 and vc_stft_power_f32 above: the plan's
 * padded window, reflect padding by N / 2 about sample 0 and about sample len - 1 (len = d_len[b] clamped to
 * [0, wav_stride]), F_b = min(n_frames[b], max_frames, 1 + len / hop) (d_n_frames NULL: without the first; a negative count
 * counts as 0) and the "short" rule: len <= N / 2 or hop * (F_b - 1) <= N / 2 gives F_b = 0.  d_frames_out [batch] int32
 * receives F_b.  The spectrum is planar and BIN-MAJOR: d_re, d_im [batch, n_bins, max_frames] float32, n_bins = 1 + N / 2
 * -- the solver walks time for one bin, and a tile of 16 frames still stores runs of 64 bytes.  Every element is written
 * once, frames at or beyond F_b as 0.  One launch, no workspace: the forward half of the filter kernels (16 frames per
 * workgroup and the 25 x 16 transform at n_fft == 400, 4 frames and the direct transform otherwise), statement for statement
 * that of vc_stft_power_f32, so that re^2 + im^2 of this launch is that launch's power up to the rounding of the two squares
 * and their sum.  VC_ERR_INVALID before the launch for a NULL pointer (d_n_frames excepted), batch outside [1, 65535],
 * max_frames < 1 or wav_stride < 1.
 *
 * vc_istft_complex_f32: y = istft(Z), the filter's inverse half: inverse transform and synthesis window into the frame
 * buffer, then the vocoder's overlap-add kernel.  F_b = d_n_frames[b] clamped to [0, max_frames] (NULL: max_frames), and 0
 * where hop * (F_b - 1) <= N / 2.  Output as vc_stft_filter_f32's: hop * (F_b - 1) samples, then zeros up to out_stride;
 * every element of d_out [batch, out_stride] is written once.  The imaginary parts of bin 0 and of bin N / 2 are IGNORED
 * (a real frame has none); nothing else of a frame at or beyond F_b is read.  Workspace: vc_stft_filter_workspace_bytes,
 * used as the filter uses it.  VC_ERR_INVALID for a NULL pointer (d_n_frames excepted), batch outside [1, 65535],
 * max_frames < 1 or out_stride < hop * (max_frames - 1); VC_ERR_WORKSPACE for a workspace that is too small.
 *
 * vc_wpe_f32: the solver.  d_re, d_im [batch, n_bins, max_frames] as above; F = d_n_frames[b] clamped to [0, max_frames]
 * (NULL: max_frames); K = taps, D = delay, I = iterations, c = context.  Per (b, k), with x_t the input bin converted to
 * float64 and xt_t[i] = x_{t - D - i}, i < K, where a term whose index t - D - i is negative is LEFT OUT of every sum below
 * (nothing is multiplied by an absent frame):
 *     m    = (sum_t |x_t|^2, t = 0 .. F - 1 ascending from +0) / F            |z|^2 = re * re + im * im
 *     lam0 = double(floor_rel) * m
 *     p_t  = |x_t|^2
 *     repeat I times:
 *         lam_t   = (sum of p_u, u = max(t - c, 0) .. min(t + c, F - 1) ascending from +0) / (number of terms);
 *                   lam_t = lam0 unless lam_t > lam0
 *         R[i][j] = sum_t (xt_t[i] * conj(xt_t[j])) / lam_t      i <= j;  t = D + j .. F - 1 ascending from +0
 *         q[i]    = sum_t (xt_t[i] * conj(x_t)) / lam_t          t = D + i .. F - 1 ascending from +0
 *                   a * conj(b) = (ar * br + ai * bi,  ai * br - ar * bi); the real and the imaginary part are each divided
 *                   by lam_t, then added to their sums
 *         tr = sum_i R[i][i].re (i ascending from +0);  R[i][i].re += (double(load_rel) * tr) / K
 *         R = L L^H, for j = 0 .. K - 1:
 *             d    = R[j][j].re - |L[j][0]|^2 - ... - |L[j][j-1]|^2          left to right; R[j][j].im is not read
 *             a pivot d that is not positive and finite ends the bin with status 1
 *             L[j][j] = sqrt(d)
 *             L[i][j] = (conj(R[j][i]) - L[i][0] * conj(L[j][0]) - ... - L[i][j-1] * conj(L[j][j-1])) / L[j][j]    i > j
 *         L z = q:    z[i] = (q[i] - L[i][0] * z[0] - ... - L[i][i-1] * z[i-1]) / L[i][i]                  i ascending
 *                     a * b = (ar * br - ai * bi,  ar * bi + ai * br)
 *         L^H g = z:  g[i] = (z[i] - conj(L[K-1][i]) * g[K-1] - ... - conj(L[i+1][i]) * g[i+1]) / L[i][i]  i descending
 *                     conj(a) * b = (ar * br + ai * bi,  ar * bi - ai * br)
 *         y_t = x_t - (sum_i conj(g[i]) * xt_t[i], i = 0 .. min(K, t - D + 1) - 1 ascending from +0);   p_t = |y_t|^2
 * Everything is float64 without contraction: a complex product is four real products and two sums, each rounded once and
 * subtracted (or added) as a whole, real and imaginary part on their own; division and square root are IEEE; a complex
 * number is divided by a real one part by part.  y stays float64 between iterations and is rounded to float32 once, at the
 * end.  d_out_re, d_out_im [batch, n_bins, max_frames]: y, frames at or beyond F as 0.  d_taps [batch, n_bins, K, 2] float32
 * (optional): the last iteration's g, (re, im).  d_status [batch, n_bins] int32: 0 solved; 1 a pivot that was not positive
 * and finite in any iteration (an all-zero bin is one: m == 0, and 0 / 0 reaches the first pivot); 2 F <= D, no history at
 * all.  With status 1 or 2 the bin is passed through -- y = x bit for bit -- and its taps are 0.  Every element of every
 * output is written exactly once.
 * Hence: scaling the input by 2^n scales the output by exactly 2^n and leaves taps and status bit-identical (R and q are
 * ratios, the floor and the load are relative; away from overflow and underflow); the result is a function of its own
 * (utterance, bin) alone, bit-identical alone, in any batch and under graph replay.
 * One launch, one workgroup per (utterance, bin): the bin's frames are staged once in LDS from the contiguous row; each of
 * the K (K + 1) / 2 sums of R and the K sums of q has one lane for its owner and walks t; the factorisation and the
 * substitutions run a lane per row, a column per step, out of LDS; lam and y take a lane per frame.  The frames live in
 * LDS, 24 bytes each behind 8 (2 K^2 + 2 K + 4) bytes of matrix, so max_frames is capped:
 *     vc_wpe_max_frames(K) = (160 KiB - 8 (2 K^2 + 2 K + 4)) / 24          6,121 at K = 32, 6,644 at K = 16 (0: K out of range)
 * VC_ERR_INVALID before the launch for a NULL pointer (d_n_frames and d_taps excepted), batch outside [1, 65535], n_bins
 * outside [2, 2049], max_frames < 1 or beyond the cap, taps outside [1, 32], delay outside [1, 64], iterations outside
 * [1, 16], context outside [0, 8], floor_rel outside (0, 1], load_rel outside [0, 1].
 *
 * None of the launches allocates, sets memory, uses atomics or synchronises; the lengths are read on the device; all are
 * capturable from the first call. */
typedef struct vc_wpe_cfg {
    int32_t taps;       /* K: length of the predictor */
    int32_t delay;      /* D: frames between the newest predicting frame and the predicted one */
    int32_t iterations; /* I: re-weighting passes */
    int32_t context;    /* c: the power is averaged over the frames t - c .. t + c */
    float floor_rel;    /* floor of the weight, relative to the bin's mean power */
    float load_rel;     /* diagonal loading, relative to the mean of the diagonal */
} vc_wpe_cfg;
int vc_stft_complex_f32(const vc_vocoder_plan* plan, const float* d_wav, int32_t wav_stride, const int32_t* d_len,
                        const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float* d_re, float* d_im,
                        int32_t* d_frames_out, void* stream);
int vc_istft_complex_f32(const vc_vocoder_plan* plan, const float* d_re, const float* d_im, const int32_t* d_n_frames,
                         int32_t batch, int32_t max_frames, float* d_out, int32_t out_stride, void* d_workspace,
                         size_t workspace_bytes, void* stream);
int32_t vc_wpe_max_frames(int32_t taps);
int vc_wpe_f32(const float* d_re, const float* d_im, const int32_t* d_n_frames, int32_t batch, int32_t n_bins, int32_t max_frames,
               const vc_wpe_cfg* cfg, float* d_out_re, float* d_out_im, float* d_taps, int32_t* d_status, void* stream);

/* Exemplar conversion.  The non-parallel route: the target speaker is a bank of their own frames, each keyed by the phoneme
 * recogniser's posterior; every source frame is replaced by the mean of the k bank frames whose posteriors are nearest
 * (PPG-based exemplar conversion; kNN-VC, Baas et al. 2023, with posteriorgrams in place of WavLM features).  The
 * Bhattacharyya coefficient sum_c sqrt(p_c q_c) of two posteriors is the dot product of their square roots; with the roots
 * in 8 bits the search is an int8 matrix product, and integer arithmetic makes EVERYTHING below exact: the device equals the
 * numpy restatement tests/exemplar_ref.py bit for bit, tie-breaks included, whatever the tiling.  Three launches
 * (csrc/vc_knn.hip), added without a version bump.
 *
 * Key.  p[c] float32 posteriors of C <= 128 classes; Kp = vc_knn_key_width(C) = 64 for C <= 64, else 128 (0: C out of range).
 *     key[c]  = p[c] > 0 ? (int8) min(127, rintf(127.0f * sqrtf(p[c]))) : 0       c < C;     key[c] = 0,  C <= c < Kp
 *     norm    = sum_c key[c]^2                                                    int32
 * The square root is correctly rounded, the product is one float32 product, rintf rounds half to even; a NaN, a negative
 * value and -0 give 0, +inf gives 127.
 * vc_ppg_key_i8: d_ppg [batch, max_frames, C] float32 and d_n_frames [batch] to d_key [batch, max_frames, Kp] int8 and d_norm
 * [batch, max_frames] int32.  A row f >= d_n_frames[b] gets the zero key and norm 0, and its posteriors are not read.  A
 * bank is keyed by the same launch (batch = 1 serves a compacted bank).  Every output element is written once.
 *
 * Distance.  d(q, j) = norm_q + norm_j - 2 * sum_c q[c] * b_j[c], int32, in [0, 4,129,024]; d / (2 * 127^2) approximates the
 * squared Hellinger distance 1 - sum_c sqrt(p_c q_c).  The distance and not the bare dot product: quantised norms vary by a
 * few per cent and a dot product favours long keys, while under the distance a key's own copy lies at 0 and nothing is
 * closer.  Key bytes must lie in [0, 127] (vc_ppg_key_i8 writes no others); with other bytes the result is unspecified,
 * though nothing is read or written out of bounds.
 *
 * Selection (vc_knn_i8).  Query row m = b * max_frames + f of d_qkey [batch * max_frames, Kp] is valid when f < d_n_frames[b].
 * Its candidates are the bank rows j in [0, n_bank) outside [excl[b][0], excl[b][1]); (0, 0) -- or no table -- excludes
 * nothing; the exclusion gives leave-one-out when the bank holds the query's own recording.  Candidates are ordered by
 * (d, j) ascending, a total order; d_idx [Mq, k] and d_dist [Mq, k] (Mq = batch * max_frames, 1 <= k <= 16) receive the first
 * k of them, slots without a candidate -1 and -1, rows that are not valid -1 throughout.  Every element of both is written
 * once.  The result is a function of the inputs alone: not of tile sizes, nor of n_splits.
 * The exclusion table is passed twice, as h_excl (host, [batch, 2] int32: the launcher checks it) and as d_excl (its device
 * copy: the kernel reads it); both or neither.  n_splits: over how many workgroup columns the bank is split; 0 leaves the
 * choice to the launcher (vc_knn_splits reports it), a positive value up to 1,024 is honoured, also beyond the number of
 * 16-row tiles of the bank (such splits are empty).  Workspace: vc_knn_workspace_bytes(Mq, n_bank, k, n_splits) bytes (0 for
 * arguments the launcher would refuse), 16-byte aligned, as are d_qkey, d_bkey and d_bnorm.
 * Two launches.  Sweep: grid (query tiles of 16 / 4, splits), one wave per query tile; v_mfma_i32_16x16x64_i8 with 16 bank
 * rows as A and the 16 queries, resident in registers and negated once, as B; lane l supplies bytes 16 (l >> 4) .. + 15 of row
 * l & 15 on both sides (and those at + 64 in a second instruction at Kp = 128), reads one query (l & 15) and the four bank
 * rows 4 (l >> 4) + reg from the accumulator, keeps a sorted list of its best in registers (1, 4, 8 or 16 long, the first
 * that holds k), and compares the minimum of its four new values with the list's last before it inserts.  The four lane
 * groups of a query exchange and merge their lists at the end and write them to the workspace [split][m][slot] as (d, j).
 * Merge: one lane per query row merges the splits' lists and writes the first k.  No LDS, no atomics.
 *
 * Mean (vc_knn_mean_f32).  d_values [n_bank, dim] float32.  The list of row m ends before the first slot i that holds an
 * index outside [0, n_bank) (-1 is one) or, for i >= 1 and d_max >= 0, a distance above d_max; n = the number of slots
 * before that (a filled slot 0 always counts; d_max < 0: no gate).
 *     out[m][c] = (((v[idx_0][c] + v[idx_1][c]) + v[idx_2][c]) + ...) / (float) n        float32 additions in slot order,
 *                                                                                         one IEEE division;  n = 0: zeros
 * d_out [n_queries, dim] float32 and d_n_used [n_queries] int32 are written once each.  One wave per row, lanes along dim.
 *
 * VC_ERR_INVALID before any launch for: a NULL pointer (the exclusion pair excepted), one of h_excl / d_excl without the
 * other, k outside [1, 16], n_classes outside [1, 128], key_width other than 64 or 128, a row count (batch * max_frames,
 * n_queries, n_bank) outside [1, 2^24], dim outside [1, 65536], n_splits outside [0, 1024], a pointer that misses its
 * alignment, an exclusion that is not 0 <= excl[b][0] <= excl[b][1] <= n_bank; VC_ERR_WORKSPACE for a workspace that is too
 * small.  None of the launches allocates, sets memory, uses atomics or synchronises; the frame counts are read on the
 * device; all are capturable from the first call. */
int32_t vc_knn_key_width(int32_t n_classes);
int vc_ppg_key_i8(const float* d_ppg, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_classes, int8_t* d_key,
                  int32_t* d_norm, void* stream);
int32_t vc_knn_splits(int32_t n_queries, int32_t n_bank, int32_t n_splits);
size_t vc_knn_workspace_bytes(int32_t n_queries, int32_t n_bank, int32_t k, int32_t n_splits);
int vc_knn_i8(const int8_t* d_qkey, const int32_t* d_qnorm, const int32_t* d_n_frames, const int32_t* h_excl, const int32_t* d_excl,
              int32_t batch, int32_t max_frames, const int8_t* d_bkey, const int32_t* d_bnorm, int32_t n_bank, int32_t key_width,
              int32_t k, int32_t n_splits, void* d_workspace, size_t workspace_bytes, int32_t* d_idx, int32_t* d_dist, void* stream);
int vc_knn_mean_f32(const int32_t* d_idx, const int32_t* d_dist, int32_t n_queries, int32_t k, int32_t d_max, const float* d_values,
                    int32_t n_bank, int32_t dim, float* d_out, int32_t* d_n_used, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VC_HIP_H */
