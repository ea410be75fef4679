// pt_adaptive.hip -- the active list of an adaptively sampled accumulator (include/pt/pt.h, pt_accum_freeze /
// pt_accum_active), for gfx950: ordered stream compaction of the per-slot frozen_at plane into the ascending list
// of the work slots still sampled.  Ascending keeps a wave's pixels of an active pass in nearby 8x8 blocks.
// Three launches, lanes on consecutive slots (one coalesced 4-B load per lane), no atomics, so the list is the
// same on every run:
//   active_count    per wave ballot + popcount, the block's 4 wave counts added through LDS -> block_tot[b]
//   active_scan     one block: exclusive scan of block_tot in place, 256 at a time with a running carry (LDS
//                   Hillis-Steele); the total lands in block_tot[nblocks]
//   active_scatter  the flag again, rank = block offset + earlier waves of the block + earlier lanes of the wave
// Separate launches order the three steps; no block reads another block's stores inside a launch.
#include <hip/hip_runtime.h>

#include "../host/host_internal.h"
#include "pt_hip_util.h"

namespace {

constexpr int kBlock = 256;   // 4 waves; one slot per lane

__global__ __launch_bounds__(kBlock) void active_count(const uint32_t* __restrict__ frozen_at, uint32_t n,
                                                       uint32_t* __restrict__ block_tot)
{
    __shared__ uint32_t wave_n[kBlock / 64];
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool active = q < n && frozen_at[q] == pt::kSlotActive;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(active));
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) block_tot[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

__global__ __launch_bounds__(kBlock) void active_scan(uint32_t* __restrict__ block_tot, uint32_t nblocks)
{
    __shared__ uint32_t s[2][kBlock];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? block_tot[i] : 0u;
        int cur = 0;
        s[0][threadIdx.x] = v;
        __syncthreads();
        for (uint32_t off = 1; off < (uint32_t)kBlock; off <<= 1) {   // inclusive scan of the 256 values
            const uint32_t x = s[cur][threadIdx.x] + (threadIdx.x >= off ? s[cur][threadIdx.x - off] : 0u);
            s[cur ^ 1][threadIdx.x] = x;
            cur ^= 1;
            __syncthreads();
        }
        const uint32_t incl = s[cur][threadIdx.x], total = s[cur][kBlock - 1];
        if (i < nblocks) block_tot[i] = carry + incl - v;
        carry += total;
        __syncthreads();   // (s is rewritten by the next round)
    }
    if (threadIdx.x == 0) block_tot[nblocks] = carry;
}

__global__ __launch_bounds__(kBlock) void active_scatter(const uint32_t* __restrict__ frozen_at, uint32_t n,
                                                         const uint32_t* __restrict__ block_off, uint32_t* __restrict__ list)
{
    __shared__ uint32_t wave_n[kBlock / 64];
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool active = q < n && frozen_at[q] == pt::kSlotActive;
    const unsigned long long m = __ballot(active);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!active) return;
    uint32_t rank = block_off[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < wave; ++k) rank += wave_n[k];
    list[rank] = q;   // rank < the total <= n: the list holds n entries
}

}  // namespace

size_t pt::adaptive_scan_words(size_t slots) { return (slots + kBlock - 1) / kBlock + 1; }

int pt::adaptive_compact(const uint32_t* frozen_at, size_t slots, uint32_t* list, uint32_t* block_tot, void* stream_v,
                         uint32_t* count)
{
    *count = 0;
    if (!slots) return PT_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const uint32_t n = (uint32_t)slots, nblocks = (uint32_t)((slots + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(active_count, dim3(nblocks), dim3(kBlock), 0, stream, frozen_at, n, block_tot);
    hipLaunchKernelGGL(active_scan, dim3(1), dim3(kBlock), 0, stream, block_tot, nblocks);
    hipLaunchKernelGGL(active_scatter, dim3(nblocks), dim3(kBlock), 0, stream, frozen_at, n, block_tot, list);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count, block_tot + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PT_OK;
}
