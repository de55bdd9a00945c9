// cs_nfsp.hip -- the NFSP agent's reservoir buffer (rlcard/agents/nfsp_agent.py ReservoirBuffer) in HBM, for every env
// of a handle at once. (The average-policy network and the per-mode row lists are k_qnet's, cs_dqn.hip.)
//
//   A push offers the window's best-response rows of the chosen seats -- the candidates, in (t, env) order -- to the
//   buffer. Candidate number pos of the push has stream index k = add_calls + pos, and ReservoirBuffer.add's slot
//   depends on k alone: slot k while k < cap (the list is still growing), afterwards j = floor(x * (k + 1) / 2^64) with
//   x the first two words of philox4(seed, k, 0) -- uniform on [0, k], np.random.randint(0, k + 1) restated -- if
//   j < cap, and no slot otherwise. The sequential algorithm therefore leaves in each slot the candidate with the
//   largest k that maps to it:
//   k_reservoir_claim   atomicMax of k + 1 into the slot's occupant word (stream indices only grow, so the word
//                       persists across pushes)
//   k_reservoir_write   the candidate whose k + 1 is the slot's word writes its row: one writer per slot, whatever
//                       the order the threads run in
//   k_reservoir_gather  slots -> f32 state rows and one-hot action_probs rows
#include "cs_device.h"
#include "cs_dqn.h"
#include "cs_scan.h"

namespace cs {

constexpr int RBLOCK = 256;

// 1 where row i of the window is a candidate (0 past the window: the scan's last entry, whose sum is the push's count)
struct ReservoirCand {
    const uint8_t* player;
    const uint8_t* mode;
    int64_t M;
    int32_t P;
    uint32_t seat_mask;
    __host__ __device__ int32_t operator()(const int64_t& i) const
    {
        if (i >= M) return 0;
        const int p = player[i];
        return (p < P && ((seat_mask >> p) & 1u) && mode[i] != 0) ? 1 : 0;
    }
};

// slot of stream index k, or -1 where the draw drops it
__device__ __forceinline__ int64_t reservoir_slot(const Reservoir& r, uint64_t k)
{
    if (k < (uint64_t)r.cap) return (int64_t)k;
    uint32_t w[4];
    philox4(r.seed, k, 0, w);
    const uint64_t x = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    const uint64_t j = __umul64hi(x, k + 1);
    return j < (uint64_t)r.cap ? (int64_t)j : -1;
}

__global__ __launch_bounds__(RBLOCK) void k_reservoir_claim(Reservoir r, ReservoirCand cand,
                                                            const int32_t* __restrict__ pos)
{
    const int64_t i = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (i >= cand.M || !cand(i)) return;
    const uint64_t k = (uint64_t)*r.add_calls + (uint64_t)pos[i];
    const int64_t slot = reservoir_slot(r, k);
    if (slot >= 0) atomicMax(r.occ + slot, (unsigned long long)(k + 1));
}

// one thread per row: past the fill phase few rows win a slot (about cap / k of the candidates), so the copy of a
// winner's O bytes by its own lane costs less than a thread per 4 bytes of every row (4-byte words where the rows are
// word aligned: obs and st are allocation-aligned, so O % 4 == 0 suffices)
__global__ __launch_bounds__(RBLOCK) void k_reservoir_write(Reservoir r, ReservoirCand cand,
                                                            const int32_t* __restrict__ pos,
                                                            const uint8_t* __restrict__ obs,
                                                            const void* __restrict__ action)
{
    const int O = r.O;
    const int64_t row = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (row >= cand.M || !cand(row)) return;
    const uint64_t k = (uint64_t)*r.add_calls + (uint64_t)pos[row];
    const int64_t slot = reservoir_slot(r, k);
    if (slot < 0 || r.occ[slot] != (unsigned long long)(k + 1)) return;
    const uint8_t* src = obs + row * O;
    uint8_t* dst = r.st + slot * O;
    if (((O | (int)(uintptr_t)obs) & 3) == 0) {
        for (int u = 0; u < O; u += 4) *(uint32_t*)(dst + u) = *(const uint32_t*)(src + u);
    } else {
        for (int u = 0; u < O; u++) dst[u] = src[u];
    }
    r.act[slot] = traj_action(action, r.abytes, row);
}

__global__ void k_reservoir_advance(Reservoir r, const int32_t* __restrict__ pos, int64_t M)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *r.add_calls += pos[M];
}

hipError_t launch_reservoir_push(const Reservoir& r, int32_t T, int64_t n, const uint8_t* obs, const uint8_t* player,
                                 const void* action, const uint8_t* mode, uint32_t seat_mask, int32_t* pos, DevBuf& scan,
                                 hipStream_t s)
{
    const int64_t M = (int64_t)T * n;
    const ReservoirCand cand{player, mode, M, r.P, seat_mask};
    hipcub::CountingInputIterator<int64_t> rows(0);
    hipcub::TransformInputIterator<int32_t, ReservoirCand, hipcub::CountingInputIterator<int64_t>> flags(rows, cand);
    hipError_t e = scan_sum(scan, flags, pos, (int)(M + 1), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_reservoir_claim, dim3((unsigned)((M + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, s, r, cand, pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_reservoir_write, dim3((unsigned)((M + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, s, r, cand, pos,
                       obs, action);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_reservoir_advance, dim3(1), dim3(64), 0, s, r, pos, M);
    return hipGetLastError();
}

// idx[k] = a slot in [0, size), size = min(add_calls, cap). One thread per (k, 4 obs units). An index outside that
// range is the caller's error; it is clamped, so the kernel reads inside the buffer whatever it is.
__global__ __launch_bounds__(RBLOCK) void k_reservoir_gather(Reservoir r, const int64_t* __restrict__ idx, int64_t B,
                                                             float* __restrict__ o_st, float* __restrict__ o_pr)
{
    const int O = r.O;
    int64_t k;
    int c0;
    if (!row_col4((int64_t)blockIdx.x * RBLOCK + threadIdx.x, B, O, k, c0)) return;
    const int64_t calls = *r.add_calls, size = calls < r.cap ? calls : r.cap;
    const int64_t slot = clamp_index(idx[k], size);
    if (o_st) {
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (c0 + u < O) o_st[k * O + c0 + u] = (float)r.st[slot * O + c0 + u];
    }
    if (c0 == 0 && o_pr) {
        const int a = r.act[slot];
        for (int u = 0; u < r.A; u++) o_pr[k * r.A + u] = u == a ? 1.f : 0.f;
    }
}

hipError_t launch_reservoir_gather(const Reservoir& r, const int64_t* idx, int64_t B, float* state, float* probs,
                                   hipStream_t s)
{
    const int64_t work = B * ((r.O + 3) / 4);
    hipLaunchKernelGGL(k_reservoir_gather, dim3((unsigned)((work + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, s, r, idx, B,
                       state, probs);
    return hipGetLastError();
}

}  // namespace cs
