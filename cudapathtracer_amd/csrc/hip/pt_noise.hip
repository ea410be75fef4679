// pt_noise.hip -- per-pixel noise estimates of a progressive render (include/pt/pt.h, pt_noise_*), for gfx950.
// The estimator watches an accumulator's f64 running mean from outside: the mean before and after a pass gives
// the mean of that pass's samples, and Welford's weighted update over those batch means gives the variance of the
// pixel mean.  No render kernel is involved.  The arithmetic is the header's, operation by operation (f64, no
// contraction, IEEE division); tests/noise_ref.py restates it in numpy and the kernels agree with it in every bit.
//
// State: five f64 planes per work slot, in the accumulator's slot order (like its mean): prev[3], mu, m2.
// Three kernels, lanes on consecutive slots, so every plane access is a coalesced 8-B-per-lane row:
//   noise_update<kFold>  one sweep: (kFold) folds the newest pass into the state, then rel2, the converged
//                        count (per wave: ballot + popcount) and a 64-bin LDS histogram per block, flushed
//                        with one global atomic per non-zero bin into one of kSumCopies copies of a small
//                        buffer, which the host adds up.  All integer: no reduction-order effects.
//   noise_map            rel2 of every slot scattered to its pixel's index (scanline or Morton).
//   noise_variance       the variance of the mean of all of the pixel's samples, scattered the same way: what the
//                        variance-guided denoiser (pt_denoise_guided) takes.
// Adaptive sampling (the accumulator has frozen pixels: AccumView::frozen_at): the pixels' counts differ, so each
// slot carries its own window weight and batch count (two u32 planes, allocated then: kPix instances of the two
// kernels; an accumulator with no frozen pixel runs the scalar instances, unchanged), and
//   noise_freeze         one sweep: rel2 from the planes, the test, the frozen_at store, and the counts of the
//                        newly frozen and the still active pixels (per wave ballot + popcount, per block through
//                        LDS, flushed into kSumCopies copies like the summary).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../host/host_internal.h"
#include "pt_hip_util.h"

namespace {

constexpr int kBlock = 256;
// grid cap: blocks per CU, the rest of the slots by grid stride.  Measured at 1920x1080: 2 / 4 / 8 /
// 16 / 32 give 39 / 34 / 35 / 35 / 36 us for the folding sweep.
constexpr uint32_t kBlocksPerCu = 4;
constexpr uint32_t kNoPixel = 0xffffffffu;
constexpr int kSumWords = 65;          // hist[64], converged
// A block flushes into copy blockIdx.x % kSumCopies of the summary buffer and the host adds the copies (integers:
// any order gives the same sums): with one copy the flush's same-address atomics were the sweep's time, which grew
// linearly with the number of blocks.
constexpr int kSumCopies = 32;

struct NoiseArgs {
    const double* mean;     // the accumulator's mean planes, mean[k * n + q]
    double* state;          // prev[3], mu, m2 planes
    const uint32_t* dst;    // slot -> index in the accumulator's pixel order, kNoPixel outside the image
    unsigned long long* sum;   // kSumCopies x kSumWords
    float* map;             // noise_map only
    size_t n;               // slots
    double n1, n0, s;       // fold: samples now, at the last fold, and their difference
    double ratio;           // fold: s / (W + s)
    double vden;            // (batches - 1) * W after the fold
    double y_floor, tol2;
    int32_t batches;        // after the fold
    // per-pixel counts (kPix): the accumulator's frozen_at plane and this estimator's W_q / b_q planes
    uint32_t* frozen_at;
    uint32_t* pw;           // W_q
    uint32_t* pb;           // b_q
    uint32_t n_now;         // noise_freeze: the active pixels' sample count
};

// rel2 of a pixel with window mean mu and weighted square sum m2 (the header's "error")
__device__ __forceinline__ double noise_rel2(const NoiseArgs& a, double mu, double m2)
{
    if (a.batches < 2) return __longlong_as_double(0x7ff0000000000000ll);
    const double var = m2 / a.vden;
    const double den = (mu > a.y_floor) ? mu : a.y_floor;
    return var / (den * den);
}
// ... with the pixel's own batch count and window weight
__device__ __forceinline__ double noise_rel2_pix(const NoiseArgs& a, double mu, double m2, uint32_t b, uint32_t w)
{
    if (b < 2u) return __longlong_as_double(0x7ff0000000000000ll);
    const double var = m2 / ((double)(b - 1u) * (double)w);
    const double den = (mu > a.y_floor) ? mu : a.y_floor;
    return var / (den * den);
}

__device__ __forceinline__ int noise_bin(float r)
{
    if (r != r) return 63;
    if (!(r > 0.0f)) return 0;
    const uint32_t bits = __float_as_uint(r);
    if (bits == 0x7f800000u) return 63;
    const int b = (int)((bits >> 23) & 255u) - 127 + 48;
    return b < 1 ? 1 : (b > 62 ? 62 : b);
}

template <bool kFold, bool kPix = false>
__global__ __launch_bounds__(kBlock) void noise_update(NoiseArgs a)
{
    __shared__ uint32_t hist[64];
    __shared__ uint32_t conv;
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    if (threadIdx.x == 64) conv = 0;
    __syncthreads();
    const size_t n = a.n;
    uint32_t wave_conv = 0;   // (wave-uniform)
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        const bool pixel = a.dst[q] != kNoPixel;
        double mu = a.state[3 * n + q], m2 = a.state[4 * n + q];
        if (kPix) {
            // the pixel's count n_q: where it was frozen, or the active pixels' n1; it folds iff n_q > n0, with
            // its own s = n_q - n0 and window weight (an active pixel: the scalar arithmetic, bit for bit)
            uint32_t w = a.pw[q], nb = a.pb[q];
            if (kFold) {
                const uint32_t at = a.frozen_at[q];
                const double nq = (at == pt::kSlotActive) ? a.n1 : (double)at;
                if (nq > a.n0) {
                    const double s = nq - a.n0;
                    double b[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double m1 = a.mean[k * n + q];
                        const double prev = a.state[k * n + q];
                        b[k] = (m1 * nq - prev * a.n0) / s;
                        a.state[k * n + q] = m1;
                    }
                    const double y = (0.2126 * b[0] + 0.7152 * b[1]) + 0.0722 * b[2];
                    const double Wn = (double)w + s;
                    const double d = y - mu;
                    mu = mu + d * (s / Wn);
                    m2 = m2 + (s * d) * (y - mu);
                    a.state[3 * n + q] = mu;
                    a.state[4 * n + q] = m2;
                    w += (uint32_t)s;
                    nb += 1u;
                    a.pw[q] = w;
                    a.pb[q] = nb;
                }
            }
            const double rel2 = noise_rel2_pix(a, mu, m2, nb, w);
            wave_conv += (uint32_t)__popcll(__ballot(pixel && rel2 <= a.tol2));
            if (pixel) atomicAdd(&hist[noise_bin((float)rel2)], 1u);
            continue;
        }
        if (kFold) {
            double b[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double m1 = a.mean[k * n + q];
                const double prev = a.state[k * n + q];
                b[k] = (m1 * a.n1 - prev * a.n0) / a.s;
                a.state[k * n + q] = m1;
            }
            const double y = (0.2126 * b[0] + 0.7152 * b[1]) + 0.0722 * b[2];
            const double d = y - mu;
            mu = mu + d * a.ratio;
            m2 = m2 + (a.s * d) * (y - mu);
            a.state[3 * n + q] = mu;
            a.state[4 * n + q] = m2;
        }
        const double rel2 = noise_rel2(a, mu, m2);
        wave_conv += (uint32_t)__popcll(__ballot(pixel && rel2 <= a.tol2));
        if (pixel) atomicAdd(&hist[noise_bin((float)rel2)], 1u);
    }
    if ((threadIdx.x & 63) == 0 && wave_conv) atomicAdd(&conv, wave_conv);
    __syncthreads();
    unsigned long long* const sum = a.sum + (blockIdx.x % kSumCopies) * kSumWords;
    if (threadIdx.x < 64) {
        if (hist[threadIdx.x]) atomicAdd(&sum[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
    } else if (threadIdx.x == 64) {
        if (conv) atomicAdd(&sum[64], (unsigned long long)conv);
    }
}

template <bool kPix>
__global__ __launch_bounds__(kBlock) void noise_map(NoiseArgs a)
{
    const size_t n = a.n;
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        const uint32_t o = a.dst[q];
        if (o == kNoPixel) continue;
        const double mu = a.state[3 * n + q], m2 = a.state[4 * n + q];
        a.map[o] = (float)(kPix ? noise_rel2_pix(a, mu, m2, a.pb[q], a.pw[q]) : noise_rel2(a, mu, m2));
    }
}

// pt_noise_variance: the variance of the mean of all n_q samples, m2 / ((b - 1) * n_q), scattered like noise_map.
// Scalar instance: a.batches and a.vden = (batches - 1) * samples; kPix: b_q from the plane, n_q the count the
// pixel was frozen at or a.n_now.
template <bool kPix>
__global__ __launch_bounds__(kBlock) void noise_variance(NoiseArgs a)
{
    const size_t n = a.n;
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        const uint32_t o = a.dst[q];
        if (o == kNoPixel) continue;
        const double m2 = a.state[4 * n + q];
        double v = __longlong_as_double(0x7ff0000000000000ll);
        if (kPix) {
            const uint32_t b = a.pb[q], at = a.frozen_at[q];
            const uint32_t nq = (at == pt::kSlotActive) ? a.n_now : at;
            if (b >= 2u) v = m2 / ((double)(b - 1u) * (double)nq);
        } else if (a.batches >= 2) {
            v = m2 / a.vden;
        }
        a.map[o] = (float)v;
    }
}

// Every slot's W_q / b_q from the scalars: until the first freeze all pixels fold in step.
__global__ __launch_bounds__(kBlock) void noise_fill_pix(NoiseArgs a, uint32_t w, uint32_t b)
{
    const size_t n = a.n;
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        a.pw[q] = w;
        a.pb[q] = b;
    }
}

// pt_noise_freeze: every active pixel with rel2 <= tol2 is frozen at the active pixels' count.  sum[0]: newly
// frozen, sum[1]: still active, in copy blockIdx.x % kSumCopies.
__global__ __launch_bounds__(kBlock) void noise_freeze(NoiseArgs a)
{
    __shared__ uint32_t cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t n = a.n;
    uint32_t wave_new = 0, wave_act = 0;   // (wave-uniform)
    for (size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kBlock) {
        const bool active = a.dst[q] != kNoPixel && a.frozen_at[q] == pt::kSlotActive;
        const double rel2 = noise_rel2_pix(a, a.state[3 * n + q], a.state[4 * n + q], a.pb[q], a.pw[q]);
        const bool freeze = active && rel2 <= a.tol2;
        if (freeze) a.frozen_at[q] = a.n_now;
        wave_new += (uint32_t)__popcll(__ballot(freeze));
        wave_act += (uint32_t)__popcll(__ballot(active && !freeze));
    }
    if ((threadIdx.x & 63) == 0) {
        if (wave_new) atomicAdd(&cnt[0], wave_new);
        if (wave_act) atomicAdd(&cnt[1], wave_act);
    }
    __syncthreads();
    unsigned long long* const sum = a.sum + (blockIdx.x % kSumCopies) * kSumWords;
    if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&sum[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

bool params_ok(const pt_noise_params* np)
{
    return std::isfinite(np->tol) && np->tol > 0.0f && std::isfinite(np->y_floor) && np->y_floor > 0.0f;
}

}  // namespace

struct pt_noise {
    pt_accum* acc = nullptr;
    pt_ctx* ctx = nullptr;
    std::vector<uint32_t> dst;          // slot -> index in the accumulator's pixel order (kNoPixel: no pixel)
    uint64_t pixels = 0;
    uint32_t* d_dst = nullptr;
    double* d_state = nullptr;          // 5 planes of slots() doubles
    unsigned long long* d_sum = nullptr;
    uint32_t* d_pix = nullptr;          // W_q and b_q planes (2 x slots()), once the accumulator has frozen pixels
    bool pix_live = false;              // the planes carry the state (else the scalars W and batches do)
    int64_t n0 = 0;                     // samples at the last fold (at first: n_start)
    double W = 0.0;                     // window weight: samples folded
    int32_t batches = 0;
    size_t slots() const { return dst.size(); }
};

namespace {

int check(const char* who, const pt_noise* z, const pt_noise_params* np)
{
    if (!z || !np) return pt::fail(PT_E_INVALID, "%s: null argument", who);
    if (!params_ok(np)) return pt::fail(PT_E_INVALID, "%s: tol and y_floor must be finite and > 0", who);
    if (pt::ctx_in_flight(z->ctx) > 0)
        return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(z->ctx));
    return PT_OK;
}

int check_variance(const char* who, const pt_noise* z, const float* var)
{
    if (!z || !var) return pt::fail(PT_E_INVALID, "%s: null argument", who);
    if (pt::ctx_in_flight(z->ctx) > 0)
        return pt::fail(PT_E_INVALID, "%s: %d asynchronous renders in flight (pt_render_wait first)", who, pt::ctx_in_flight(z->ctx));
    return PT_OK;
}

unsigned grid_of(const pt_noise* z)
{
    const size_t blocks = (z->slots() + kBlock - 1) / kBlock;
    // PT_NOISE_BLOCKS_PER_CU: the grid cap, for measurements (default kBlocksPerCu)
    const char* v = getenv("PT_NOISE_BLOCKS_PER_CU");
    const int per_cu = (v && *v) ? atoi(v) : 0;
    const size_t cap = (size_t)pt::ctx_num_cus(z->ctx) * (per_cu >= 1 && per_cu <= 64 ? (uint32_t)per_cu : kBlocksPerCu);
    return (unsigned)(blocks < cap ? blocks : cap);
}

// The arguments of a summary / map at the estimator's current state.
NoiseArgs args_of(const pt_noise* z, const pt_noise_params* np)
{
    NoiseArgs a;
    memset(&a, 0, sizeof(a));
    a.mean = pt::accum_view(z->acc).mean;
    a.state = z->d_state;
    a.dst = z->d_dst;
    a.sum = z->d_sum;
    a.n = z->slots();
    a.batches = z->batches;
    a.vden = (double)(z->batches - 1) * z->W;
    a.y_floor = (double)np->y_floor;
    a.tol2 = (double)np->tol * (double)np->tol;
    a.frozen_at = const_cast<uint32_t*>(pt::accum_view(z->acc).frozen_at);
    a.pw = z->d_pix;
    a.pb = z->d_pix ? z->d_pix + z->slots() : nullptr;
    return a;
}

// Per-pixel counts from now on (the accumulator has frozen pixels, or pt_noise_freeze is about to freeze some):
// the W_q / b_q planes, filled from the scalars that described every pixel until now.
int go_per_pixel(pt_noise* z, hipStream_t stream)
{
    if (z->pix_live) return PT_OK;
    const size_t n = z->slots() ? z->slots() : 1;
    if (!z->d_pix) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&z->d_pix), 2 * n * sizeof(uint32_t)));
    if (z->slots()) {
        NoiseArgs a;
        memset(&a, 0, sizeof(a));
        a.n = z->slots();
        a.pw = z->d_pix;
        a.pb = z->d_pix + z->slots();
        hipLaunchKernelGGL(noise_fill_pix, dim3(grid_of(z)), dim3(kBlock), 0, stream, a, (uint32_t)z->W, (uint32_t)z->batches);
        HIP_TRY(hipGetLastError());
    }
    z->pix_live = true;
    return PT_OK;
}
// ... as soon as the accumulator has a frozen pixel (every entry point asks first)
int follow_accum(pt_noise* z, hipStream_t stream)
{
    return pt::accum_view(z->acc).frozen_at ? go_per_pixel(z, stream) : PT_OK;
}

}  // namespace

// ---- session files (pt_session.cpp): the estimator's window as it stands, and an estimator that continues one
void pt::noise_session(pt_noise* z, pt::SessionNoise* out)
{
    *out = pt::SessionNoise{z->d_state, z->pix_live ? z->d_pix : nullptr, z->n0, z->W, z->batches};
}

pt_noise* pt::noise_session_new(pt_accum* acc, int64_t n0, double W, int32_t batches, bool per_pixel, int* code)
{
    pt_noise* z = pt_noise_create(acc, code);
    if (!z) return nullptr;
    z->n0 = n0;
    z->W = W;
    z->batches = batches;
    if (per_pixel) {
        const size_t n = z->slots() ? z->slots() : 1;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&z->d_pix), 2 * n * sizeof(uint32_t));
        if (e != hipSuccess) {
            *code = pt::fail(PT_E_HIP, "pt_session_load: hipMalloc of the W_q / b_q planes failed: %s", hipGetErrorString(e));
            pt_noise_destroy(z);
            return nullptr;
        }
        z->pix_live = true;
    }
    return z;
}

extern "C" {

void pt_noise_defaults(pt_noise_params* p)
{
    if (!p) return;
    p->tol = 0.05f;
    p->y_floor = 0.01f;
}

pt_noise* pt_noise_create(pt_accum* acc, int* err)
{
    pt::clear_error();
    pt_noise* z = nullptr;
    auto make = [&]() -> int {
        if (!acc) return pt::fail(PT_E_INVALID, "pt_noise_create: null accumulator");
        const pt::AccumView v = pt::accum_view(acc);
        if (*v.noise) return pt::fail(PT_E_INVALID, "pt_noise_create: the accumulator already has a live estimator");
        if (pt::ctx_in_flight(v.ctx) > 0)
            return pt::fail(PT_E_INVALID, "pt_noise_create: %d asynchronous renders in flight (pt_render_wait first)", pt::ctx_in_flight(v.ctx));
        z = new (std::nothrow) pt_noise();
        if (!z) return pt::fail(PT_E_OOM, "pt_noise_create: out of host memory");
        z->acc = acc;
        z->ctx = v.ctx;
        z->n0 = v.samples;
        const uint32_t w = (uint32_t)v.params->width;
        z->dst = *v.slot_pix;
        for (uint32_t& o : z->dst) {
            if (o == kNoPixel) continue;
            ++z->pixels;
            if (v.params->pixel_order == PT_ORDER_MORTON) o = pt_morton_pxl_to_i(o % w, o / w);
        }
        const size_t n = z->slots() ? z->slots() : 1;
        HIP_TRY(hipSetDevice(pt::ctx_device(v.ctx)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&z->d_dst), n * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&z->d_state), n * 5 * sizeof(double)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&z->d_sum), kSumCopies * kSumWords * sizeof(unsigned long long)));
        if (z->slots()) {
            HIP_TRY(hipMemcpy(z->d_dst, z->dst.data(), z->slots() * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(z->d_state, v.mean, z->slots() * 3 * sizeof(double), hipMemcpyDeviceToDevice));   // prev = the mean
        }
        HIP_TRY(hipMemset(z->d_state + 3 * z->slots(), 0, (n * 5 - 3 * z->slots()) * sizeof(double)));          // mu = m2 = 0
        HIP_TRY(hipDeviceSynchronize());
        *v.noise = z;
        return PT_OK;
    };
    const int code = make();
    if (code != PT_OK && z) {
        pt_noise_destroy(z);
        z = nullptr;
    }
    if (err) *err = code;
    return z;
}

int pt_noise_update(pt_noise* z, const pt_noise_params* np, void* stream_v, pt_noise_summary* out)
{
    pt::clear_error();
    if (!out) return pt::fail(PT_E_INVALID, "pt_noise_update: null argument");
    if (int rc = check("pt_noise_update", z, np)) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const int64_t n1 = pt::accum_view(z->acc).samples;
    const bool fold = n1 > z->n0;
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    if (int rc = follow_accum(z, stream)) return rc;
    NoiseArgs a = args_of(z, np);
    if (fold) {
        const double s = (double)(n1 - z->n0), Wn = z->W + s;
        a.n1 = (double)n1; a.n0 = (double)z->n0; a.s = s;
        a.ratio = s / Wn;
        a.batches = z->batches + 1;
        a.vden = (double)(a.batches - 1) * Wn;
    }
    unsigned long long part[kSumCopies * kSumWords], sum[kSumWords];
    memset(part, 0, sizeof(part));
    if (z->slots()) {
        HIP_TRY(hipMemsetAsync(z->d_sum, 0, sizeof(part), stream));
        if (z->pix_live) {
            if (fold) hipLaunchKernelGGL((noise_update<true, true>), dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
            else hipLaunchKernelGGL((noise_update<false, true>), dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
        }
        else if (fold) hipLaunchKernelGGL((noise_update<true>), dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
        else hipLaunchKernelGGL((noise_update<false>), dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(part, z->d_sum, sizeof(part), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    for (int k = 0; k < kSumWords; ++k) {
        sum[k] = 0;
        for (int c = 0; c < kSumCopies; ++c) sum[k] += part[c * kSumWords + k];
    }
    if (fold) {   // (a failed launch above leaves the window as it was)
        z->W += (double)(n1 - z->n0);
        z->n0 = n1;
        z->batches += 1;
    }
    out->samples = n1;
    out->batches = z->batches;
    out->pixels = z->pixels;
    out->converged = sum[64];
    for (int k = 0; k < 64; ++k) out->hist[k] = sum[k];
    return PT_OK;
}

int pt_noise_map_device(pt_noise* z, const pt_noise_params* np, float* d_rel2, void* stream_v)
{
    pt::clear_error();
    if (!d_rel2) return pt::fail(PT_E_INVALID, "pt_noise_map_device: null argument");
    if (int rc = check("pt_noise_map_device", z, np)) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    if (!z->slots()) return PT_OK;
    if (int rc = follow_accum(z, stream)) return rc;
    NoiseArgs a = args_of(z, np);
    a.map = d_rel2;
    if (z->pix_live) hipLaunchKernelGGL(noise_map<true>, dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(noise_map<false>, dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

int pt_noise_map(pt_noise* z, const pt_noise_params* np, float* rel2)
{
    pt::clear_error();
    if (!rel2) return pt::fail(PT_E_INVALID, "pt_noise_map: null argument");
    if (int rc = check("pt_noise_map", z, np)) return rc;
    const pt_params* p = pt::accum_view(z->acc).params;
    const size_t bytes = (size_t)p->width * (size_t)p->height * sizeof(float);
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    pt::ScopedDevice<float> d;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), bytes));
    HIP_TRY(hipMemset(d, 0, bytes));
    if (int rc = pt_noise_map_device(z, np, d, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rel2, d, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_noise_variance_device(pt_noise* z, float* d_var, void* stream_v)
{
    pt::clear_error();
    if (int rc = check_variance("pt_noise_variance_device", z, d_var)) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    if (!z->slots()) return PT_OK;
    if (int rc = follow_accum(z, stream)) return rc;
    pt_noise_params np;
    pt_noise_defaults(&np);   // (unused by the kernel: the variance has no floor and no tolerance)
    NoiseArgs a = args_of(z, &np);
    const int64_t samples = pt::accum_view(z->acc).samples;
    a.map = d_var;
    a.vden = (double)(z->batches - 1) * (double)samples;
    a.n_now = (uint32_t)samples;
    if (z->pix_live) hipLaunchKernelGGL(noise_variance<true>, dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(noise_variance<false>, dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}

int pt_noise_variance(pt_noise* z, float* var)
{
    pt::clear_error();
    if (int rc = check_variance("pt_noise_variance", z, var)) return rc;
    const pt_params* p = pt::accum_view(z->acc).params;
    const size_t bytes = (size_t)p->width * (size_t)p->height * sizeof(float);
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    pt::ScopedDevice<float> d;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), bytes));
    HIP_TRY(hipMemset(d, 0, bytes));
    if (int rc = pt_noise_variance_device(z, d, nullptr)) return rc;
    HIP_TRY(hipMemcpy(var, d, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_noise_freeze(pt_noise* z, const pt_noise_params* np, void* stream_v, uint64_t* newly_frozen, uint64_t* active)
{
    pt::clear_error();
    if (!newly_frozen || !active) return pt::fail(PT_E_INVALID, "pt_noise_freeze: null argument");
    if (int rc = check("pt_noise_freeze", z, np)) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    const pt::AccumView v = pt::accum_view(z->acc);
    *newly_frozen = 0;
    *active = 0;
    if (!z->slots()) return PT_OK;
    uint32_t* plane = nullptr;
    if (int rc = pt::accum_freeze_plane(z->acc, &plane)) return rc;
    if (int rc = go_per_pixel(z, stream)) return rc;
    NoiseArgs a = args_of(z, np);
    a.frozen_at = plane;
    a.n_now = (uint32_t)v.samples;
    unsigned long long part[kSumCopies * kSumWords];
    HIP_TRY(hipMemsetAsync(z->d_sum, 0, sizeof(part), stream));
    hipLaunchKernelGGL(noise_freeze, dim3(grid_of(z)), dim3(kBlock), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(part, z->d_sum, sizeof(part), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int c = 0; c < kSumCopies; ++c) {
        *newly_frozen += part[c * kSumWords];
        *active += part[c * kSumWords + 1];
    }
    pt::accum_frozen(z->acc, *newly_frozen);
    // (nothing frozen on an accumulator without frozen pixels: it stays on the scalar path, and the planes are
    // filled again when they are next needed)
    if (!pt::accum_view(z->acc).frozen_at) z->pix_live = false;
    return PT_OK;
}

int pt_noise_read(pt_noise* z, double* mu, double* m2)
{
    pt::clear_error();
    if (!z) return pt::fail(PT_E_INVALID, "pt_noise_read: null estimator");
    const pt_params* p = pt::accum_view(z->acc).params;
    const size_t n = z->slots(), npix = (size_t)p->width * (size_t)p->height;
    std::vector<double> st(2 * n);
    HIP_TRY(hipSetDevice(pt::ctx_device(z->ctx)));
    if (n) HIP_TRY(hipMemcpy(st.data(), z->d_state + 3 * n, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
    if (mu) memset(mu, 0, npix * sizeof(double));
    if (m2) memset(m2, 0, npix * sizeof(double));
    for (size_t q = 0; q < n; ++q) {
        const uint32_t o = z->dst[q];
        if (o == kNoPixel) continue;
        if (mu) mu[o] = st[q];
        if (m2) m2[o] = st[n + q];
    }
    return PT_OK;
}

void pt_noise_destroy(pt_noise* z)
{
    if (!z) return;
    (void)hipSetDevice(pt::ctx_device(z->ctx));
    if (z->d_dst) (void)hipFree(z->d_dst);
    if (z->d_state) (void)hipFree(z->d_state);
    if (z->d_sum) (void)hipFree(z->d_sum);
    if (z->d_pix) (void)hipFree(z->d_pix);
    pt_noise** slot = pt::accum_view(z->acc).noise;
    if (*slot == z) *slot = nullptr;
    delete z;
}

}  // extern "C"
