// One translation unit of liboct_unet_hip.so (see host.hpp): the Keras optimizer family with gradient clipping
// (kernels_opt.hpp) and its C ABI: oct_opt_slot_count, oct_opt_scratch_bytes, oct_opt_step (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_opt.hpp"

using namespace oct;
using namespace octh;

static_assert(K_SGD == OCT_OPT_SGD && K_ADAM == OCT_OPT_ADAM && K_ADAMAX == OCT_OPT_ADAMAX && K_RMSPROP == OCT_OPT_RMSPROP &&
              K_ADAGRAD == OCT_OPT_ADAGRAD && K_ADADELTA == OCT_OPT_ADADELTA, "kernel kinds follow the ABI's");
static_assert(kNormParts <= kBlock && kNormPartsGlobal <= kBlock, "opt_scale_k sums a variable's partials in one block");
static_assert(CLIP_NONE == OCT_CLIP_NONE && CLIP_VALUE == OCT_CLIP_VALUE && CLIP_NORM == OCT_CLIP_NORM &&
              CLIP_GLOBAL == OCT_CLIP_GLOBAL_NORM, "clip modes follow the ABI's");

namespace {

// the kernel variant (V_A | V_B bits of kernels_opt.hpp) a descriptor selects, or -1
int variant(const oct_opt_desc& d) {
    switch (d.kind) {
    case OCT_OPT_SGD:     return d.momentum != 0.f ? (V_A | ((d.flags & OCT_OPT_NESTEROV) ? V_B : 0)) : 0;   // Keras: no momentum, no nesterov
    case OCT_OPT_ADAM:    return (d.flags & OCT_OPT_AMSGRAD) ? V_A : 0;
    case OCT_OPT_RMSPROP: return (d.momentum != 0.f ? V_A : 0) | ((d.flags & OCT_OPT_CENTERED) ? V_B : 0);
    case OCT_OPT_ADAMAX: case OCT_OPT_ADAGRAD: case OCT_OPT_ADADELTA: return 0;
    default: return -1;
    }
}

int slot_count(const oct_opt_desc& d) {
    const int v = variant(d);
    switch (d.kind) {
    case OCT_OPT_SGD:     return v & V_A ? 1 : 0;
    case OCT_OPT_ADAM:    return v & V_A ? 3 : 2;
    case OCT_OPT_RMSPROP: return 1 + ((v & V_A) ? 1 : 0) + ((v & V_B) ? 1 : 0);
    case OCT_OPT_ADAGRAD: return 1;
    case OCT_OPT_ADAMAX: case OCT_OPT_ADADELTA: return 2;
    default: return -1;
    }
}

size_t global_parts(size_t n) { return std::max<size_t>(1, std::min<size_t>(kNormPartsGlobal, (n + 4095) / 4096)); }
size_t round16(size_t b) { return (b + 15) / 16 * 16; }
// scratch layout: double part[max(n_vars * kNormParts, global_parts(n))], then float scale[max(n_vars, 1)]
size_t part_count(size_t n_vars, size_t n) { return std::max(n_vars * kNormParts, global_parts(n)); }

template <int KIND, int V>
void launch(const OptArgs& a, int grid, hipStream_t st) { opt_k<KIND, V><<<grid, kBlock, 0, st>>>(a); }

}  // namespace

int oct_opt_slot_count(const oct_opt_desc* desc) {
    if (!desc || variant(*desc) < 0) { fail(-1, "opt_slot_count: bad descriptor"); return -1; }
    return slot_count(*desc);
}

size_t oct_opt_scratch_bytes(size_t n_vars, size_t n) {
    return round16(part_count(n_vars, n) * sizeof(double)) + round16(std::max<size_t>(n_vars, 1) * sizeof(float));
}

int oct_opt_step(const oct_opt_desc* desc, float* p, const float* g, float* const* slots, size_t n, long step,
                 const unsigned long long* var_off_dev, size_t n_vars, void* scratch_dev, oct_stream_t stream) {
    if (!desc || !p || !g || step < 1) return fail(-1, "opt_step: null descriptor / params / grads, or step < 1");
    const oct_opt_desc& d = *desc;
    const int v = variant(d);
    if (v < 0) return fail(-1, "opt_step: unknown optimizer kind " + std::to_string(d.kind));
    const int ns = slot_count(d);
    if (ns > 0 && !slots) return fail(-1, "opt_step: this optimizer needs state buffers (oct_opt_slot_count)");
    for (int k = 0; k < ns; ++k)
        if (!slots[k]) return fail(-1, "opt_step: state buffer " + std::to_string(k) + " is null");
    if (d.clip_mode < OCT_CLIP_NONE || d.clip_mode > OCT_CLIP_GLOBAL_NORM) return fail(-1, "opt_step: unknown clip_mode");
    const bool by_norm = d.clip_mode == OCT_CLIP_NORM || d.clip_mode == OCT_CLIP_GLOBAL_NORM;
    if (d.clip_mode != OCT_CLIP_NONE && !(by_norm ? d.clip > 0.f : d.clip >= 0.f) )
        return fail(-1, "opt_step: the clipping threshold must be positive (clipvalue: not negative)");
    if (by_norm && (!scratch_dev || (uintptr_t)scratch_dev % 16)) return fail(-1, "opt_step: clipping by norm needs 16-byte aligned scratch");
    if (d.clip_mode == OCT_CLIP_NORM && (!var_off_dev || n_vars < 1 || n_vars > 0x7fffffffu / kNormParts))
        return fail(-1, "opt_step: OCT_CLIP_NORM needs the variable table");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;

    OptArgs a{};
    a.p = p; a.g = g; a.n = n;
    for (int k = 0; k < ns; ++k) a.s[k] = slots[k];
    a.b1 = d.beta1; a.b2 = d.beta2; a.rho = d.rho; a.mu = d.momentum; a.eps = d.eps;
    a.clip_mode = d.clip_mode; a.clip = d.clip;
    // step-dependent factors in double, as oct_adam_step forms them
    double lr = (double)d.lr;
    if (d.kind == OCT_OPT_ADAM)
        lr = lr * std::sqrt(1.0 - std::pow((double)d.beta2, (double)step)) / (1.0 - std::pow((double)d.beta1, (double)step));
    else if (d.kind == OCT_OPT_ADAMAX)
        lr = lr / (1.0 - std::pow((double)d.beta1, (double)step));
    a.lr = (float)lr;
    // float4 accesses where every buffer reaches 16-byte alignment at the same element
    const uintptr_t mis = (uintptr_t)p % 16;
    bool vec = mis % 4 == 0 && (uintptr_t)g % 16 == mis;
    for (int k = 0; k < ns; ++k) vec = vec && (uintptr_t)a.s[k] % 16 == mis;
    a.head = vec ? std::min<size_t>(n, (16 - mis) % 16 / 4) : n;
    a.nvec = (n - a.head) / 4;

    if (by_norm) {
        const bool per_var = d.clip_mode == OCT_CLIP_NORM;
        const size_t nv = per_var ? n_vars : 1;
        const unsigned parts = per_var ? kNormParts : (unsigned)global_parts(n);
        double* part = (double*)scratch_dev;
        float* scale = (float*)((char*)scratch_dev + round16(part_count(n_vars, n) * sizeof(double)));
        if (nv > 65535) return fail(-1, "opt_step: more than 65535 variables");
        opt_sqnorm_k<<<dim3(parts, (unsigned)nv), kBlock, 0, st>>>(g, n, per_var ? var_off_dev : nullptr, part);
        HIP_OK(hipGetLastError());
        opt_scale_k<<<(unsigned)nv, kBlock, 0, st>>>(part, (int)parts, d.clip, scale);
        HIP_OK(hipGetLastError());
        a.var_off = per_var ? var_off_dev : nullptr; a.n_vars = (int)nv; a.scale = scale;
    }

    const size_t work = a.nvec + (n - 4 * a.nvec);
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((work + kBlock - 1) / kBlock, 4096));
    switch (d.kind * 4 + v) {
    case OCT_OPT_SGD * 4:                   launch<K_SGD, 0>(a, grid, st); break;
    case OCT_OPT_SGD * 4 + V_A:             launch<K_SGD, V_A>(a, grid, st); break;
    case OCT_OPT_SGD * 4 + (V_A | V_B):     launch<K_SGD, V_A | V_B>(a, grid, st); break;
    case OCT_OPT_ADAM * 4:                  launch<K_ADAM, 0>(a, grid, st); break;
    case OCT_OPT_ADAM * 4 + V_A:            launch<K_ADAM, V_A>(a, grid, st); break;
    case OCT_OPT_ADAMAX * 4:                launch<K_ADAMAX, 0>(a, grid, st); break;
    case OCT_OPT_RMSPROP * 4:               launch<K_RMSPROP, 0>(a, grid, st); break;
    case OCT_OPT_RMSPROP * 4 + V_A:         launch<K_RMSPROP, V_A>(a, grid, st); break;
    case OCT_OPT_RMSPROP * 4 + V_B:         launch<K_RMSPROP, V_B>(a, grid, st); break;
    case OCT_OPT_RMSPROP * 4 + (V_A | V_B): launch<K_RMSPROP, V_A | V_B>(a, grid, st); break;
    case OCT_OPT_ADAGRAD * 4:               launch<K_ADAGRAD, 0>(a, grid, st); break;
    case OCT_OPT_ADADELTA * 4:              launch<K_ADADELTA, 0>(a, grid, st); break;
    default: return fail(-1, "opt_step: no kernel for this descriptor");
    }
    HIP_OK(hipGetLastError());
    return 0;
}
