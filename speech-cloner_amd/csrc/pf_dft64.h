// 64-point real DFT building blocks for the postfilter kernels (vc_postfilter.hip): the periodic Hann window, the
// transform of a real segment into bins 0 .. 32 and the inverse for one half of the samples.
//
// z[k] = v[2k] + i v[2k+1]; a 32-point complex transform as two of fe_dft400.h's 16-point ones (even and odd k) joined by
// W32^k; then X[m] = E[m] + W64^m O[m] with E, O the transforms of the even and the odd samples, untangled from Z[m] and
// conj Z[32 - m].  The inverse runs the same steps backwards.  Every loop is unrolled and every index a constant, so the
// arrays are registers.  Plain inline C++ usable from host code too, like fe_dft400.h.
#pragma once
#include "fe_dft400.h"

namespace vcpf {

// w[t] = 0.5 - 0.5 cos(2 pi t / 64), rounded from float64
constexpr float WIN[64] = {
    0.0f, 0.0024076366639015356f, 0.0096073597983847847f, 0.021529832133895588f, 0.038060233744356631f, 0.059039367825822475f,
    0.084265193848727382f, 0.1134947733186315f, 0.14644660940672621f, 0.18280335791817726f, 0.22221488349019886f,
    0.2643016315870011f, 0.30865828381745508f, 0.35485766137276886f, 0.40245483899193585f, 0.45099142983521961f, 0.5f,
    0.54900857016478033f, 0.5975451610080641f, 0.64514233862723103f, 0.69134171618254481f, 0.73569836841299885f,
    0.77778511650980098f, 0.81719664208182263f, 0.85355339059327373f, 0.88650522668136844f, 0.91573480615127267f,
    0.94096063217417747f, 0.96193976625564337f, 0.97847016786610441f, 0.99039264020161522f, 0.99759236333609835f, 1.0f,
    0.99759236333609846f, 0.99039264020161522f, 0.97847016786610452f, 0.96193976625564348f, 0.94096063217417747f,
    0.91573480615127267f, 0.88650522668136855f, 0.85355339059327384f, 0.81719664208182297f, 0.77778511650980109f,
    0.73569836841299896f, 0.69134171618254514f, 0.64514233862723125f, 0.59754516100806432f, 0.54900857016478022f, 0.5f,
    0.45099142983521995f, 0.40245483899193585f, 0.35485766137276897f, 0.30865828381745497f, 0.26430163158700121f,
    0.22221488349019908f, 0.1828033579181772f, 0.14644660940672632f, 0.11349477331863167f, 0.084265193848727382f,
    0.059039367825822586f, 0.038060233744356742f, 0.021529832133895588f, 0.0096073597983848402f, 0.0024076366639015356f};
// cos and sin of 2 pi m / 64, m = 0 .. 32
constexpr float COS64[33] = {
    1.0f, 0.99518472667219693f, 0.98078528040323043f, 0.95694033573220882f, 0.92387953251128674f, 0.88192126434835505f,
    0.83146961230254524f, 0.77301045336273699f, 0.70710678118654757f, 0.63439328416364549f, 0.55557023301960229f,
    0.47139673682599781f, 0.38268343236508984f, 0.29028467725446233f, 0.19509032201612833f, 0.09801714032956077f, 0.0f,
    -0.098017140329560645f, -0.19509032201612819f, -0.29028467725446216f, -0.38268343236508973f, -0.4713967368259977f,
    -0.55557023301960196f, -0.63439328416364538f, -0.70710678118654746f, -0.77301045336273699f, -0.83146961230254535f,
    -0.88192126434835494f, -0.92387953251128674f, -0.95694033573220882f, -0.98078528040323043f, -0.99518472667219682f, -1.0f};
constexpr float SIN64[33] = {
    0.0f, 0.098017140329560604f, 0.19509032201612825f, 0.29028467725446233f, 0.38268343236508978f, 0.47139673682599764f,
    0.55557023301960218f, 0.63439328416364549f, 0.70710678118654746f, 0.77301045336273699f, 0.83146961230254524f,
    0.88192126434835494f, 0.92387953251128674f, 0.95694033573220894f, 0.98078528040323043f, 0.99518472667219682f, 1.0f,
    0.99518472667219693f, 0.98078528040323043f, 0.95694033573220894f, 0.92387953251128674f, 0.88192126434835505f,
    0.83146961230254546f, 0.7730104533627371f, 0.70710678118654757f, 0.63439328416364549f, 0.55557023301960218f,
    0.47139673682599786f, 0.38268343236508989f, 0.29028467725446239f, 0.19509032201612861f, 0.098017140329560826f, 0.0f};

// Complex 32-point DFT, natural order in and out: k = 2 q + p, the even and the odd inputs through cdft16, joined by
// W32^k = exp(-2 pi i k / 32).
VC_HD void cdft32(const float* zr, const float* zi, float* Zr, float* Zi) {
    float er[16], ei[16], orr[16], oi[16], ar[16], ai[16], br[16], bi[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { er[q] = zr[2 * q]; ei[q] = zi[2 * q]; orr[q] = zr[2 * q + 1]; oi[q] = zi[2 * q + 1]; }
    vcfe::cdft16(er, ei, ar, ai);
    vcfe::cdft16(orr, oi, br, bi);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float tr = br[k], ti = bi[k];
        if (k > 0) vcfe::cmul(tr, ti, COS64[2 * k], -SIN64[2 * k]);
        Zr[k] = ar[k] + tr; Zi[k] = ai[k] + ti;
        Zr[k + 16] = ar[k] - tr; Zi[k + 16] = ai[k] - ti;
    }
}

// The same, but only outputs [16 * HALF, 16 * HALF + 16) are formed (written to Zr / Zi [0, 16)).
template <int HALF>
VC_HD void cdft32_half(const float* zr, const float* zi, float* Zr, float* Zi) {
    float er[16], ei[16], orr[16], oi[16], ar[16], ai[16], br[16], bi[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { er[q] = zr[2 * q]; ei[q] = zi[2 * q]; orr[q] = zr[2 * q + 1]; oi[q] = zi[2 * q + 1]; }
    vcfe::cdft16(er, ei, ar, ai);
    vcfe::cdft16(orr, oi, br, bi);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float tr = br[k], ti = bi[k];
        if (k > 0) vcfe::cmul(tr, ti, COS64[2 * k], -SIN64[2 * k]);
        Zr[k] = HALF ? ar[k] - tr : ar[k] + tr;
        Zi[k] = HALF ? ai[k] - ti : ai[k] + ti;
    }
}

// Real 64-point DFT, bins 0 .. 32.
VC_HD void rdft64(const float* v, float* xr, float* xi) {
    float zr[32], zi[32], Zr[32], Zi[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) { zr[k] = v[2 * k]; zi[k] = v[2 * k + 1]; }
    cdft32(zr, zi, Zr, Zi);
#pragma unroll
    for (int m = 0; m <= 32; ++m) {
        const int km = m & 31, kn = (32 - m) & 31;
        const float Er = 0.5f * (Zr[km] + Zr[kn]), Ei = 0.5f * (Zi[km] - Zi[kn]);
        const float Or = 0.5f * (Zi[km] + Zi[kn]), Oi = 0.5f * (Zr[kn] - Zr[km]);
        xr[m] = Er + (Or * COS64[m] + Oi * SIN64[m]);
        xi[m] = Ei + (Oi * COS64[m] - Or * SIN64[m]);
    }
}

// Inverse of rdft64 (with the 1 / 64) for samples [32 * HALF, 32 * HALF + 32) alone.  Im Y[0] and Im Y[32] are taken as
// they come (the callers hand over 0 times something).
template <int HALF>
VC_HD void irdft64_half(const float* yr, const float* yi, float* out) {
    float zr[32], zi[32], Zr[16], Zi[16];
#pragma unroll
    for (int m = 0; m < 32; ++m) {
        const int n = 32 - m;
        const float Er = yr[m] + yr[n], Ei = yi[m] - yi[n];
        const float Dr = yr[m] - yr[n], Di = yi[m] + yi[n];
        const float Or = Dr * COS64[m] - Di * SIN64[m], Oi = Dr * SIN64[m] + Di * COS64[m];
        zr[m] = Er - Oi;                    // Z = E + i O, handed over conjugated: idft(Z) = conj(dft(conj Z))
        zi[m] = -(Ei + Or);
    }
    cdft32_half<HALF>(zr, zi, Zr, Zi);
#pragma unroll
    for (int k = 0; k < 16; ++k) { out[2 * k] = Zr[k] * (1.0f / 64.0f); out[2 * k + 1] = Zi[k] * (-1.0f / 64.0f); }
}

}  // namespace vcpf
