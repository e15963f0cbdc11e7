// libvc_hip.so: version / error plumbing shared by all entry points (include/vc_hip.h).
#include <cstdarg>
#include <atomic>
#include <cstdio>
#include <cstring>
#include "vc_common.h"

namespace vc {

static thread_local char g_err[512] = "";

char* last_error_buf() { return g_err; }

int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static std::atomic<int> g_opt[OPT_COUNT];
static const struct { const char* name; Option id; } k_opts[] = {
    {"bank256", OPT_BANK256}, {"bank256_xcd", OPT_BANK256_XCD}, {"conv256", OPT_CONV256},
    {"conv256_min_k", OPT_CONV256_MINK}, {"conv256_wm", OPT_CONV256_WM}, {"proj256", OPT_PROJ256}, {"proj256_split", OPT_PROJ256_SPLIT},
    {"wgrad_xcd", OPT_WGRAD_XCD}, {"gru_mfma", OPT_GRU_MFMA}, {"fe_fused", OPT_FE_FUSED},
    {"fe_fused_spin", OPT_FE_FUSED_SPIN}, {"gru_train_resident", OPT_GRU_TRAIN_RESIDENT},
    {"prenet_lds", OPT_PRENET_LDS}, {"cbhg_front_mi", OPT_CBHG_FRONT_MI}, {"gemm16_split", OPT_GEMM16_SPLIT},
    {"f32_f16x3", OPT_F32_F16X3}, {"gru_f32_wide", OPT_GRU_F32_WIDE},
};
static struct OptInit { OptInit() { for (auto& o : g_opt) o.store(-1); } } g_opt_init;

int opt(Option o) { return g_opt[o].load(std::memory_order_relaxed); }

static __global__ void zero_words_kernel(unsigned* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

hipError_t zero_async(void* d_p, size_t bytes, hipStream_t st) {
    if (bytes % 4) return hipErrorInvalidValue;
    const size_t n = bytes / 4;
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st,
                       static_cast<unsigned*>(d_p), n);
    return hipGetLastError();
}

}  // namespace vc

extern "C" {

int vc_set_option(const char* name, int value) {
    VC_REQUIRE(name, "vc_set_option: NULL name");
    for (const auto& o : vc::k_opts)
        if (!std::strcmp(o.name, name)) {
            vc::g_opt[o.id].store(value);
            return VC_OK;
        }
    return vc::set_error(VC_ERR_INVALID, "vc_set_option: unknown option %s", name);
}

int vc_get_option(const char* name, int* value) {
    VC_REQUIRE(name && value, "vc_get_option: NULL argument");
    for (const auto& o : vc::k_opts)
        if (!std::strcmp(o.name, name)) { *value = vc::g_opt[o.id].load(); return VC_OK; }
    return vc::set_error(VC_ERR_INVALID, "vc_get_option: unknown option %s", name);
}

int vc_version(void) { return VC_ABI_VERSION; }
const char* vc_last_error(void) { return vc::last_error_buf(); }
const char* vc_target_arch(void) { return "gfx950"; }

}  // extern "C"
