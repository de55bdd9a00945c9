// cs_dqn.hip -- the DQN agent's device side (rlcard/agents/dqn_agent.py), for every env of a handle at once:
//
//   k_qnet            DQNAgent.predict / step / eval_step: the Q-network (eval-mode BatchNorm folded into the first
//                     Linear by the caller, then Linear/tanh layers and the output Linear) for 64 obs rows per block,
//                     masked by the legal bitmask, with the first-maximum argmax and k_dmc_select's epsilon draw fused
//                     in. fp32 FMAs with fp32 accumulation in input-unit order, no MFMA (fp32 MFMA runs at the vector
//                     rate on gfx950, and bf16 would cost the fp32 agreement with the torch network).
//                       layout: the block's activations live in LDS, transposed [unit][row], two buffers (in and out of
//                       a layer, swapped per layer) sized by the widths they hold. A hidden layer is computed in tiles
//                       of 64 rows x 64 output units by one wave, each lane an 8 x 8 register tile: per input unit two
//                       16-B LDS reads of 8 activations and two of 8 weights feed 64 FMAs, so neither the LDS pipe nor
//                       a load's latency bounds the loop (a first version with one row per lane, 8 outputs per
//                       activation read and the weights by scalar loads waited on the scalar cache: 1.37 ms for 2^20
//                       Leduc rows against this one's 0.64, profiles/EXPERIMENTS.md D-1). The weights of a tile come
//                       through a per-wave LDS stage of 16 input units, loaded coalesced (16 lanes per weight row) into
//                       registers while the previous stage's FMAs run. A net with a layer wider than 64 units runs two
//                       waves per block, one per tile of the layer. The output layer (<= 8 actions) is one pass with a
//                       lane per row, its weights staged once, and stays in registers for the mask and the argmax.
//                       A game of 9..64 actions (UNO: 61, 240 obs bytes) takes the WIDE instantiations: the obs rows
//                       stay the bytes they are, transposed [unit][row] (8 rows of a unit are one 8-B read, converted
//                       in the first layer's loop), in the buffer that layer 1's outputs take over afterwards;
//                       the output layer is one more 64 x 64 tile through the same loop without an activation, and
//                       the head reads its row's column of that tile from LDS.
//                     The same kernel is NFSP's average-policy network (rlcard/agents/nfsp_agent.py): a template on the
//                     hidden activation (tanh | ReLU), the head (masked argmax + epsilon draw | softmax, remove_illegal
//                     and a sampled action) and an optional row list; the tiling and the staging are shared.
//   k_row_lists       cs_nfsp_actions: the rows of each mode compacted into an index list (positions from a prefix sum
//                     over the mode bytes), so that each network's instantiation runs over its own rows only.
//   k_replay_index / k_replay_write / k_replay_carry
//                     reorganize (rlcard/utils/utils.py:153-179) of a trajectory window into the replay ring, with the
//                     rows whose game runs past the window carried as one pending row per (env, seat) and completed by
//                     a later push. Write positions come from one prefix sum over [pending (env, seat)] + [rows (t, env)].
//   k_replay_gather   Memory.sample's stacking, u8 -> f32 fused.
//   k_dqn_targets     dqn_agent.py:205-218: Double-DQN best next action and target, each operation rounded to fp32.
#include <math.h>
#include "cs_device.h"
#include "cs_dqn.h"
#include "cs_scan.h"

namespace cs {

constexpr int QOC = 8;        // the most actions of the narrow head: its output layer is one register pass of 8 units
constexpr int QWIDE = 64;     // the most actions of the wide head: its output layer is one more tile of 64 units
constexpr int QBS = 72;       // bytes per input unit in the wide obs image: 64 rows + 8 (8-B aligned units; the staging
                              // lanes' byte writes, four units apart, spread over 8 banks where 64 B would give one)
constexpr int QROWS = 64;     // rows per block of k_qnet: one wave, or two that split a layer's 64-unit tiles
constexpr int QKT = 16;       // input units per staged weight tile
constexpr int QWS = 68;       // floats per input unit in the weight tile: 64 output units + 4 (16-B aligned rows whose
                              // 16 staging lanes of one output unit land on different banks)
constexpr int QWT = QKT * QWS;   // floats of the weight tile (the output layer's [in <= 128][8] image fits too)
constexpr int QBLOCK = 256;   // block of the streaming kernels
constexpr int QMAXP = 10;     // players per env (cs_traj.hip MAXP)

// weights W[ot + o][kt + k], o < 64, k < QKT, of one tile into registers: element lane + 64 s is (o, k) = (that >> 4,
// that & 15), so 16 consecutive lanes read 64 consecutive bytes of one weight row; zeros past the matrix
__device__ __forceinline__ void qnet_tile_load(const float* __restrict__ W, int in, int out, int ot, int kt, int lane,
                                               float (&pre)[QKT])
{
#pragma unroll
    for (int s = 0; s < QKT; s++) {
        const int idx = lane + 64 * s, o = ot + (idx >> 4), k = kt + (idx & 15);
        pre[s] = (o < out && k < in) ? W[(int64_t)o * in + k] : 0.f;
    }
}

// ACT: the hidden layers' activation; HEAD: what the output lane does with its row. LIST: the block's rows are
// idx[row0 ..] of the first *count entries of a row list (launch_nfsp_actions) -- whole obs rows are gathered, and the
// row's mask, done byte, draw key and outputs are those of row idx[r]; without it row r is row r.
enum { Q_TANH = 0, Q_RELU = 1 };
enum { Q_ARGMAX = 0, Q_SOFTMAX = 1 };

template <int ACT>
__device__ __forceinline__ float qnet_act(float x)
{
    if constexpr (ACT == Q_RELU) return fmaxf(x, 0.f);
    else return tanhf(x);
}

// The head of a game of up to 64 actions, run by wave 0 with a lane per row on the output tile col[a * 64 + lane]: the
// narrow head's semantics (below) with the mask a 64-bit word of (A + 7) / 8 bytes per row, bits >= A ignored. img is
// the other activation buffer, free by now: without a row list the block's q / probs rows are laid out there as
// [row][A], the 64 A contiguous floats of the output, and stored by consecutive lanes; a listed row is its own segment.
template <int HEAD, bool LIST>
__device__ __forceinline__ void qnet_head_wide(float* xo, float* img, int A, const uint8_t* __restrict__ legal,
                                               const uint8_t* __restrict__ done, int64_t rows, int64_t row0, int lane,
                                               float eps, uint64_t seed, uint64_t t, uint64_t row_base,
                                               int32_t* __restrict__ actions, float* __restrict__ q,
                                               const int32_t* __restrict__ idx)
{
    const int64_t row = row0 + lane;
    const bool live = row < rows;
    int64_t orow = row;
    if constexpr (LIST) orow = live ? idx[row] : 0;
    const int LB = (A + 7) >> 3;
    const uint64_t all = A >= 64 ? ~0ull : (1ull << A) - 1ull;
    uint64_t mask = all;
    if (legal && live) {
        mask = 0;
        for (int b = 0; b < LB; b++) mask |= (uint64_t)legal[orow * LB + b] << (8 * b);
        mask &= all;
    }
    float* col = xo + lane;
    float* mine = img + lane * A;
    int pick = -1;
    if constexpr (HEAD == Q_SOFTMAX) {
        // the narrow head's chain in id order, the probabilities kept in the row's column between the passes
        float mx = col[0];
        for (int a = 1; a < A; a++) mx = fmaxf(mx, col[a * QROWS]);
        float sum = 0.f;
        for (int a = 0; a < A; a++) {
            const float p = expf(col[a * QROWS] - mx);
            col[a * QROWS] = p;
            sum += p;
        }
        float lsum = 0.f;
        for (int a = 0; a < A; a++) {
            const float p = (mask >> a) & 1ull ? col[a * QROWS] / sum : 0.f;
            col[a * QROWS] = p;
            lsum += p;
        }
        const float uni = 1.0f / (float)__popcll(mask);
        uint32_t r[4] = {0, 0, 0, 0};
        if (actions) philox4(seed, row_base + (uint64_t)orow, t, r);
        const float u = (float)(r[2] >> 8) * (1.0f / 16777216.0f);
        int last = -1;
        float c = 0.f;
        for (int a = 0; a < A; a++) {
            const bool lg = (mask >> a) & 1ull;
            const float p = lg ? (lsum == 0.f ? uni : col[a * QROWS] / lsum) : 0.f;
            if (q) {
                if constexpr (LIST) {
                    if (live) q[orow * A + a] = p;
                } else mine[a] = p;
            }
            if (lg) {
                c = c + p;
                last = a;
                if (pick < 0 && u < c) pick = a;
            }
        }
        if (pick < 0) pick = last;   // (rounding left the sum below u)
    } else {
        float bv = 0.f;
        for (int a = 0; a < A; a++) {
            const bool lg = (mask >> a) & 1ull;
            const float v = col[a * QROWS];
            if (lg && (pick < 0 || v > bv)) {
                pick = a;
                bv = v;
            }
            if (q) {
                if constexpr (LIST) {
                    if (live) q[orow * A + a] = lg ? v : -INFINITY;
                } else mine[a] = lg ? v : -INFINITY;
            }
        }
        if (actions && pick >= 0 && eps > 0.f) {   // k_dmc_select's draw (cs_dmc.hip)
            uint32_t r[4];
            philox4(seed, row_base + (uint64_t)orow, t, r);
            const float u = (float)(r[0] >> 8) * (1.0f / 16777216.0f);
            if (u < eps) {
                int kth = (int)(((uint64_t)r[1] * (uint64_t)__popcll(mask)) >> 32);
                uint64_t m = mask;
                while (kth-- > 0) m &= m - 1;
                pick = __builtin_ctzll(m);
            }
        }
    }
    if constexpr (!LIST) {
        if (q) {   // (the wave's own LDS writes, read back in program order)
            __builtin_amdgcn_wave_barrier();
            const int64_t left = rows - row0;
            const int n = (int)(left < QROWS ? left : QROWS) * A;
            float* dst = q + row0 * A;
            for (int e = lane; e < n; e += QROWS) dst[e] = img[e];
        }
    }
    if (!actions || !live) return;
    if (done && done[orow]) pick = -1;
    actions[orow] = pick;
}

// WIDE: a game of more than 8 actions or more than 128 obs bytes -- the byte obs image and the wide head.
template <int ACT, int HEAD, bool LIST, bool WIDE = false>
__global__ __launch_bounds__(2 * QROWS) void k_qnet(const cs_qnet net, int szA, int szB, const uint8_t* __restrict__ obs,
                                                const uint8_t* __restrict__ legal, const uint8_t* __restrict__ done,
                                                int64_t rows, float eps, uint64_t seed, uint64_t t, uint64_t row_base,
                                                int32_t* __restrict__ actions, float* __restrict__ q,
                                                const int32_t* __restrict__ idx, const int32_t* __restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) float q_lds[];
    const int tid = (int)threadIdx.x, BT = (int)blockDim.x, lane = tid & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), NW = BT >> 6;   // this wave of the block's 1 or 2
    const int64_t row0 = (int64_t)blockIdx.x * QROWS;
    if constexpr (LIST) {   // the grid covers `rows`; the list holds *count of them (every thread reads the same word,
        rows = *count;      // so a block past the list leaves as one, before any barrier)
        if (row0 >= rows) return;
    }
    const int64_t row = row0 + lane;
    const int D = net.in_dim, A = net.num_actions, NH = net.num_hidden;
    float* bufA = q_lds;                  // [szA][64]: the obs rows, then the outputs of layers 1, 3
    float* bufB = bufA + szA * QROWS;     // [szB][64]: the outputs of layers 0, 2
    float* wt0 = bufB + szB * QROWS;      // [NW][QKT][QWS]: a weight tile per wave, input-unit major
    float* wt = wt0 + wv * QWT;
    if constexpr (WIDE) {
        // obs rows of the block -> bufA as the bytes they are, [unit][QBS] (qnet_sizes counts them into szA; layer 1
        // overwrites them once layer 0 has read them). Consecutive lanes take consecutive dwords of the block's rows
        // (bytes where the rows are not dword-aligned), (row, unit) stepped along without a division per element.
        uint8_t* xb = (uint8_t*)bufA;
        const int64_t left = rows - row0;
        const int nr = (int)(left < QROWS ? left : QROWS);
        const int G = (((D & 3) | (int)((uintptr_t)obs & 3)) == 0) ? 4 : 1, DG = D / G;
        const int dr = BT / DG, du = BT - dr * DG;
        int r = tid / DG, u = tid - r * DG;
        while (r < nr) {
            int64_t srow = row0 + r;
            if constexpr (LIST) srow = idx[srow];
            const uint8_t* src = obs + srow * D + u * G;
            if (G == 4) {
                const uint32_t w = *(const uint32_t*)src;
#pragma unroll
                for (int i = 0; i < 4; i++) xb[(u * 4 + i) * QBS + r] = (uint8_t)(w >> (8 * i));
            } else xb[u * QBS + r] = *src;
            r += dr;
            u += du;
            if (u >= DG) {
                u -= DG;
                r++;
            }
        }
    } else {   // obs rows of the block -> bufA as floats: consecutive lanes, consecutive bytes
        const int64_t left = rows - row0;
        const int nb = (int)(left < QROWS ? left : QROWS) * D;
        const uint8_t* src = obs + row0 * D;
        for (int j = tid; j < nb; j += BT) {
            const int r = j / D, u = j - r * D;
            if constexpr (LIST) bufA[u * QROWS + r] = (float)obs[(int64_t)idx[row0 + r] * D + u];
            else bufA[u * QROWS + r] = (float)src[j];
        }
    }
    const int lr = lane & 7, lo = lane >> 3;   // the lane's 8 rows (8 lr ..) and 8 output units (8 lo ..) of a tile
    float* xin = bufA;
    float* xout = bufB;
    int in = D;
    // (wide: the output layer is one more pass of the loop, a tile of A units -- the staging gives units A.. zero
    // weights, and they are not stored -- without an activation, [action][row] into the free buffer)
    for (int l = 0; l < (WIDE ? NH + 1 : NH); l++) {
        const int out = WIDE && l == NH ? A : net.hidden[l];
        const float* __restrict__ W = net.W[l];
        const float* __restrict__ bias = net.b[l];
        for (int ot0 = 0; ot0 < out; ot0 += 64 * NW) {   // (every wave passes the barriers; one without a tile idles)
            const int ot = ot0 + 64 * wv;
            const bool mine = ot < out;
            float acc[8][8];   // [output unit][row]
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int o = ot + lo * 8 + j;
                const float b = bias[o < out ? o : out - 1];
#pragma unroll
                for (int i = 0; i < 8; i++) acc[j][i] = b;
            }
            float pre[QKT];
            if (mine) qnet_tile_load(W, in, out, ot, 0, lane, pre);
            for (int kt = 0; kt < in; kt += QKT) {
                __syncthreads();   // the tile's readers (and, first, the writers of xin) are done
                if (mine) {
#pragma unroll
                    for (int s = 0; s < QKT; s++) {
                        const int idx = lane + 64 * s;
                        wt[(idx & 15) * QWS + (idx >> 4)] = pre[s];
                    }
                }
                __syncthreads();
                if (!mine) continue;
                if (kt + QKT < in) qnet_tile_load(W, in, out, ot, kt + QKT, lane, pre);   // in flight under the FMAs
                const int kn = in - kt < QKT ? in - kt : QKT;
                if (WIDE && l == 0) {   // the obs bytes: 8 rows of a unit are one 8-B read
#pragma unroll 2
                    for (int k = 0; k < kn; k++) {
                        const uint2 x = *(const uint2*)((const uint8_t*)xin + (kt + k) * QBS + lr * 8);
                        const float4 w0 = *(const float4*)(wt + k * QWS + lo * 8);
                        const float4 w1 = *(const float4*)(wt + k * QWS + lo * 8 + 4);
                        const float a[8] = {(float)(x.x & 255u), (float)((x.x >> 8) & 255u),
                                            (float)((x.x >> 16) & 255u), (float)(x.x >> 24),
                                            (float)(x.y & 255u), (float)((x.y >> 8) & 255u),
                                            (float)((x.y >> 16) & 255u), (float)(x.y >> 24)};
                        const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                        for (int j = 0; j < 8; j++)
#pragma unroll
                            for (int i = 0; i < 8; i++) acc[j][i] = fmaf(w[j], a[i], acc[j][i]);
                    }
                    continue;
                }
#pragma unroll 2
                for (int k = 0; k < kn; k++) {
                    const float4 a0 = *(const float4*)(xin + (kt + k) * QROWS + lr * 8);
                    const float4 a1 = *(const float4*)(xin + (kt + k) * QROWS + lr * 8 + 4);
                    const float4 w0 = *(const float4*)(wt + k * QWS + lo * 8);
                    const float4 w1 = *(const float4*)(wt + k * QWS + lo * 8 + 4);
                    const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                    for (int j = 0; j < 8; j++)
#pragma unroll
                        for (int i = 0; i < 8; i++) acc[j][i] = fmaf(w[j], a[i], acc[j][i]);
                }
            }
            const bool act = !(WIDE && l == NH);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int o = ot + lo * 8 + j;
                if (o < out) {
                    float* d = xout + o * QROWS + lr * 8;
                    if (!act) {
                        *(float4*)d = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
                        *(float4*)(d + 4) = make_float4(acc[j][4], acc[j][5], acc[j][6], acc[j][7]);
                        continue;
                    }
                    *(float4*)d = make_float4(qnet_act<ACT>(acc[j][0]), qnet_act<ACT>(acc[j][1]),
                                              qnet_act<ACT>(acc[j][2]), qnet_act<ACT>(acc[j][3]));
                    *(float4*)(d + 4) = make_float4(qnet_act<ACT>(acc[j][4]), qnet_act<ACT>(acc[j][5]),
                                                    qnet_act<ACT>(acc[j][6]), qnet_act<ACT>(acc[j][7]));
                }
            }
        }
        float* nx = xin;
        xin = xout;
        xout = nx;
        in = out;
    }
    if constexpr (WIDE) {   // wave 0, a lane per row, on its column of the output tile (xin after the last swap)
        __syncthreads();
        if (wv != 0) return;
        qnet_head_wide<HEAD, LIST>(xin, xout, A, legal, done, rows, row0, lane, eps, seed, t, row_base, actions, q, idx);
        return;
    }
    // output layer, one lane per row: its weights as wt[k][8] (zeros past A), read back as two broadcast float4
    __syncthreads();
    {
        const float* __restrict__ W = net.W[NH];
        for (int idx = tid; idx < in * QOC; idx += BT) {
            const int k = idx >> 3, a = idx & 7;
            wt0[idx] = a < A ? W[(int64_t)a * in + k] : 0.f;
        }
    }
    __syncthreads();
    if (wv != 0) return;
    float acc[QOC];
#pragma unroll
    for (int k = 0; k < QOC; k++) acc[k] = net.b[NH][k < A ? k : A - 1];
    for (int k = 0; k < in; k++) {
        const float x = xin[k * QROWS + lane];
        const float4 w0 = *(const float4*)(wt0 + k * QOC), w1 = *(const float4*)(wt0 + k * QOC + 4);
        const float w[QOC] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int j = 0; j < QOC; j++) acc[j] = fmaf(w[j], x, acc[j]);
    }
    if (row >= rows) return;
    int64_t orow = row;   // the row the mask, the done byte, the draw key and the outputs belong to
    if constexpr (LIST) orow = idx[row];
    const uint32_t all = (1u << A) - 1u;
    const uint32_t mask = legal ? (uint32_t)legal[orow] & all : all;   // A <= 8: one mask byte per row
    if constexpr (HEAD == Q_SOFTMAX) {
        // AveragePolicyNetwork + NFSPAgent._act + remove_illegal: np.exp(log_softmax) over every action, the illegal
        // entries zeroed, the rest divided by their sum (uniform over the legal actions where that sum underflowed)
        float mx = acc[0];
#pragma unroll
        for (int k = 1; k < QOC; k++)
            if (k < A) mx = fmaxf(mx, acc[k]);
        float p[QOC], sum = 0.f;
#pragma unroll
        for (int k = 0; k < QOC; k++) {
            p[k] = k < A ? expf(acc[k] - mx) : 0.f;
            sum += p[k];
        }
        float lsum = 0.f;
#pragma unroll
        for (int k = 0; k < QOC; k++) {
            p[k] = (mask >> k) & 1u ? p[k] / sum : 0.f;
            lsum += p[k];
        }
        const float uni = 1.0f / (float)__popc(mask);
#pragma unroll
        for (int k = 0; k < QOC; k++)
            if ((mask >> k) & 1u) p[k] = lsum == 0.f ? uni : p[k] / lsum;
        if (q) {
#pragma unroll
            for (int k = 0; k < QOC; k++)
                if (k < A) q[orow * A + k] = p[k];
        }
        if (!actions) return;
        // the first legal action whose running sum passes u (third Philox word: the epsilon draw takes the first two)
        uint32_t r[4];
        philox4(seed, row_base + (uint64_t)orow, t, r);
        const float u = (float)(r[2] >> 8) * (1.0f / 16777216.0f);
        int pick = -1, last = -1;
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < QOC; k++)
            if ((mask >> k) & 1u) {
                c = c + p[k];
                last = k;
                if (pick < 0 && u < c) pick = k;
            }
        if (pick < 0) pick = last;   // (rounding left the sum below u)
        if (done && done[orow]) pick = -1;
        actions[orow] = pick;
    } else {
        if (q) {
#pragma unroll
            for (int k = 0; k < QOC; k++)
                if (k < A) q[orow * A + k] = (mask >> k) & 1u ? acc[k] : -INFINITY;
        }
        if (!actions) return;
        int best = -1;
        float bv = 0.f;
#pragma unroll
        for (int k = 0; k < QOC; k++)
            if (((mask >> k) & 1u) && (best < 0 || acc[k] > bv)) {
                best = k;
                bv = acc[k];
            }
        if (best >= 0 && eps > 0.f) {   // k_dmc_select's draw (cs_dmc.hip)
            uint32_t r[4];
            philox4(seed, row_base + (uint64_t)orow, t, r);
            const float u = (float)(r[0] >> 8) * (1.0f / 16777216.0f);
            if (u < eps) {
                int kth = (int)(((uint64_t)r[1] * (uint64_t)__popc(mask)) >> 32);
                uint32_t m = mask;
                while (kth-- > 0) m &= m - 1;
                best = __builtin_ctz(m);
            }
        }
        if (done && done[orow]) best = -1;
        actions[orow] = best;
    }
}

// the wide instantiations: more actions than the narrow head's register pass, or more obs units than fit as floats
static bool qnet_wide(const cs_qnet& net) { return net.num_actions > QOC || net.in_dim > 128; }

// units ([64] floats each) of the two activation buffers. Wide: the output tile lands in one of them and the head's
// [row][A] image of q / probs in the other, so each holds 64 units at least, and bufA the obs bytes ([in_dim][QBS])
static void qnet_sizes(const cs_qnet& net, int* szA, int* szB)
{
    const bool wide = qnet_wide(net);
    int a = wide ? QWIDE : net.in_dim, b = wide ? QWIDE : 1;
    for (int l = 0; l < net.num_hidden; l++) {
        int& dst = (l & 1) ? a : b;
        if (net.hidden[l] > dst) dst = net.hidden[l];
    }
    if (wide) {
        const int ob = (net.in_dim * QBS + QROWS * 4 - 1) / (QROWS * 4);
        if (ob > a) a = ob;
    }
    *szA = a;
    *szB = b;
}

// waves of a k_qnet block: a second one where a layer is wider than one 64-unit tile
static int qnet_waves(const cs_qnet& net)
{
    for (int l = 0; l < net.num_hidden; l++)
        if (net.hidden[l] > 64) return 2;
    return 1;
}

int64_t qnet_lds_bytes(const cs_qnet& net)
{
    int a, b;
    qnet_sizes(net, &a, &b);
    return (((int64_t)a + b) * QROWS + qnet_waves(net) * QWT) * (int64_t)sizeof(float);
}

template <int ACT, int HEAD, bool LIST>
static hipError_t launch_net(const cs_qnet& net, const uint8_t* obs, const uint8_t* legal, const uint8_t* done,
                             int64_t rows, float eps, uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions,
                             float* out, const int32_t* idx, const int32_t* count, hipStream_t s)
{
    int szA, szB;
    qnet_sizes(net, &szA, &szB);
    const int64_t bytes = qnet_lds_bytes(net);
    auto kern = qnet_wide(net) ? k_qnet<ACT, HEAD, LIST, true> : k_qnet<ACT, HEAD, LIST, false>;
    if (bytes > 65536) {   // past the default limit of dynamic LDS (the [128, 128, ..] nets, any on Mahjong): raise it
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + QROWS - 1) / QROWS)), dim3(QROWS * qnet_waves(net)),
                       (size_t)bytes, s, net, szA, szB, obs, legal, done, rows, eps, seed, t, row_base, actions, out,
                       idx, count);
    return hipGetLastError();
}

hipError_t launch_qnet(const cs_qnet& net, const uint8_t* obs, const uint8_t* legal, const uint8_t* done, int64_t rows,
                       float eps, uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions, float* q,
                       hipStream_t s)
{
    return launch_net<Q_TANH, Q_ARGMAX, false>(net, obs, legal, done, rows, eps, seed, t, row_base, actions, q, nullptr,
                                               nullptr, s);
}

// the same descriptor read as Linear/ReLU with the average-policy head: probs (may be NULL) f32 [rows][A], actions
// (may be NULL) the sampled ones
hipError_t launch_pnet(const cs_qnet& net, const uint8_t* obs, const uint8_t* legal, const uint8_t* done, int64_t rows,
                       uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions, float* probs, hipStream_t s)
{
    return launch_net<Q_RELU, Q_SOFTMAX, false>(net, obs, legal, done, rows, 0.f, seed, t, row_base, actions, probs,
                                                nullptr, nullptr, s);
}

// ---- NFSP: each network on its own rows ------------------------------------------------------------------------------
// Scratch of launch_nfsp_actions, all i32: pos [rows] (exclusive sum of the mode bytes), list0 [rows] (average-policy
// rows, ascending), list1 [rows] (best-response rows), counts [2], then the scan's temporary storage.
struct ModeFlag {
    __host__ __device__ int32_t operator()(const uint8_t& m) const { return m ? 1 : 0; }
};

__global__ __launch_bounds__(QBLOCK) void k_row_lists(const uint8_t* __restrict__ mode, int64_t rows,
                                                      const int32_t* __restrict__ pos, int32_t* __restrict__ list0,
                                                      int32_t* __restrict__ list1, int32_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * QBLOCK + threadIdx.x;
    if (i >= rows) return;
    const int32_t ones = pos[i];   // mode-1 rows before row i
    const bool br = mode[i] != 0;
    if (br) list1[ones] = (int32_t)i;
    else list0[i - ones] = (int32_t)i;
    if (i == rows - 1) {
        const int32_t c1 = ones + (br ? 1 : 0);
        counts[0] = (int32_t)rows - c1;
        counts[1] = c1;
    }
}

static size_t nfsp_lists_bytes(int64_t rows)
{
    return (((size_t)rows * 3 + 2) * sizeof(int32_t) + 255) / 256 * 256;
}

hipError_t nfsp_scratch_bytes(int64_t rows, size_t* bytes)
{
    hipcub::TransformInputIterator<int32_t, ModeFlag, const uint8_t*> flags(nullptr, ModeFlag());
    size_t need = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, flags, (int32_t*)nullptr, (int)rows, (hipStream_t)0);
    if (e != hipSuccess) return e;
    *bytes = nfsp_lists_bytes(rows) + need + 256;
    return hipSuccess;
}

hipError_t launch_nfsp_actions(const cs_qnet& qnet, const cs_qnet& pnet, const uint8_t* obs, const uint8_t* legal,
                               const uint8_t* done, const uint8_t* mode, int64_t rows, float eps, uint64_t seed,
                               uint64_t t, uint64_t row_base, int32_t* actions, float* probs, void* scratch,
                               hipStream_t s)
{
    int32_t* pos = (int32_t*)scratch;
    int32_t* list0 = pos + rows;
    int32_t* list1 = list0 + rows;
    int32_t* counts = list1 + rows;
    size_t total = 0;   // the caller's scratch, by the contract of nfsp_scratch_bytes
    hipError_t e = nfsp_scratch_bytes(rows, &total);
    if (e != hipSuccess) return e;
    const size_t lists = nfsp_lists_bytes(rows);
    hipcub::TransformInputIterator<int32_t, ModeFlag, const uint8_t*> flags(mode, ModeFlag());
    if ((e = scan_sum((uint8_t*)scratch + lists, total - lists, flags, pos, (int)rows, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_row_lists, dim3((unsigned)((rows + QBLOCK - 1) / QBLOCK)), dim3(QBLOCK), 0, s, mode, rows, pos,
                       list0, list1, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_net<Q_RELU, Q_SOFTMAX, true>(pnet, obs, legal, done, rows, 0.f, seed, t, row_base, actions, probs, list0,
                                            counts, s);
    if (e != hipSuccess) return e;
    return launch_net<Q_TANH, Q_ARGMAX, true>(qnet, obs, legal, done, rows, eps, seed, t, row_base, actions, nullptr,
                                              list1, counts + 1, s);
}

// ---- replay ring ---------------------------------------------------------------------------------------------------
// Codes of an entry (a pending (env, seat) or a trajectory row): >= 0 the row of the next state (obs[code][e]);
// <= -3 the game ended first, at row -3 - code (final_obs there); -2 still running past the window; -1 not a transition.
struct ReplayCount {
    __host__ __device__ int32_t operator()(const int32_t& c) const { return (c >= 0 || c <= -3) ? 1 : 0; }
};

// One lane per env, its T rows scanned backwards (as k_transitions): code of every row of a seat in seat_mask, the
// code that completes each seat's pending row (code[e * P + q]), and the row that becomes the seat's new pending row.
__global__ __launch_bounds__(QBLOCK) void k_replay_index(const uint8_t* __restrict__ player,
                                                         const uint8_t* __restrict__ done, int T, int64_t n, int P,
                                                         uint32_t seat_mask, const uint8_t* __restrict__ pvalid,
                                                         int32_t* __restrict__ code, int32_t* __restrict__ newpend)
{
    const int64_t e = (int64_t)blockIdx.x * QBLOCK + threadIdx.x;
    if (e == 0) code[n * P + (int64_t)T * n] = -1;   // the scan's last entry: its exclusive sum is the push's total
    if (e >= n) return;
    int32_t nxt[QMAXP], np_[QMAXP];
#pragma unroll
    for (int k = 0; k < QMAXP; k++) {
        nxt[k] = -2;
        np_[k] = -1;
    }
    int32_t* rows = code + n * P;
    for (int t = T - 1; t >= 0; t--) {
        const int64_t row = (int64_t)t * n + e;
        if (done[row]) {
#pragma unroll
            for (int k = 0; k < QMAXP; k++) nxt[k] = -3 - t;
        }
        const int p = player[row];
        int32_t c = -1;
#pragma unroll
        for (int k = 0; k < QMAXP; k++) {
            if (k == p && k < P) {
                if ((seat_mask >> k) & 1u) {
                    c = nxt[k];
                    if (c == -2) np_[k] = t;
                }
                nxt[k] = t;
            }
        }
        rows[row] = c;
    }
#pragma unroll
    for (int k = 0; k < QMAXP; k++) {
        if (k < P) {
            code[e * P + k] = pvalid[e * P + k] ? nxt[k] : -1;
            newpend[e * P + k] = np_[k];
        }
    }
}

// One thread per (entry, 4 obs bytes): entry j < n * P is the pending row of (env, seat) j, the others are the window's
// rows. The entry's transition lands in slot (total + pos[j]) % cap; of a push with more than cap transitions only the
// last cap are written, so no two entries share a slot.
__global__ __launch_bounds__(QBLOCK) void k_replay_write(ReplayRing r, int T, int64_t n, const uint8_t* __restrict__ obs,
                                                         const uint8_t* __restrict__ legal,
                                                         const uint8_t* __restrict__ player,
                                                         const void* __restrict__ action,
                                                         const float* __restrict__ reward,
                                                         const uint8_t* __restrict__ final_obs,
                                                         const int32_t* __restrict__ code,
                                                         const int32_t* __restrict__ pos)
{
    const int O = r.O, P = r.P;
    const int64_t NP = n * P, M = NP + (int64_t)T * n;
    int64_t j;
    int c0;
    if (!row_col4((int64_t)blockIdx.x * QBLOCK + threadIdx.x, M, O, j, c0)) return;
    const int32_t c = code[j];
    if (!(c >= 0 || c <= -3)) return;
    const int64_t fresh = pos[M], at = pos[j];
    if (at < fresh - r.cap) return;
    const int64_t slot = (*r.total + at) % r.cap;
    int64_t e;
    int p, a;
    const uint8_t* s_src;
    if (j < NP) {
        e = j / P;
        p = (int)(j - e * P);
        s_src = r.pst + j * O;
        a = r.pact[j];
    } else {
        const int64_t row = j - NP;
        e = row % n;
        p = player[row];
        s_src = obs + row * O;
        a = traj_action(action, r.abytes, row);
    }
    const bool ended = c < 0;
    const int64_t nrow = (int64_t)(ended ? -3 - c : c) * n + e;
    const uint8_t* n_src = ended ? final_obs + (nrow * P + p) * O : obs + nrow * O;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (c0 + k < O) {
            r.st[slot * O + c0 + k] = s_src[c0 + k];
            r.nst[slot * O + c0 + k] = n_src[c0 + k];
        }
    }
    if (c0 == 0) {
        r.act[slot] = a;
        r.rew[slot] = ended ? reward[nrow * P + p] : 0.f;
        r.dne[slot] = ended ? 1 : 0;
        for (int k = 0; k < r.LB; k++) r.nlg[slot * r.LB + k] = ended ? (uint8_t)0 : legal[nrow * r.LB + k];
    }
}

// After the write: the rows that stay pending move into the (env, seat) pending store (one thread per (env, seat, 4 obs
// bytes)), completed ones are cleared, and the ring's total advances by the push's count.
__global__ __launch_bounds__(QBLOCK) void k_replay_carry(ReplayRing r, int T, int64_t n, const uint8_t* __restrict__ obs,
                                                         const void* __restrict__ action,
                                                         const int32_t* __restrict__ code,
                                                         const int32_t* __restrict__ pos)
{
    const int O = r.O;
    const int64_t NP = n * r.P;
    const int64_t i = (int64_t)blockIdx.x * QBLOCK + threadIdx.x;
    if (i == 0) *r.total += pos[NP + (int64_t)T * n];
    int64_t j;
    int c0;
    if (!row_col4(i, NP, O, j, c0)) return;
    const int32_t t = r.newpend[j];
    if (t < 0) {
        const int32_t c = code[j];
        if (c0 == 0 && (c >= 0 || c <= -3)) r.pvalid[j] = 0;
        return;
    }
    const int64_t row = (int64_t)t * n + j / r.P;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (c0 + k < O) r.pst[j * O + c0 + k] = obs[row * O + c0 + k];
    if (c0 == 0) {
        r.pact[j] = traj_action(action, r.abytes, row);
        r.pvalid[j] = 1;
    }
}

hipError_t launch_replay_push(const Buffers& b, const ReplayRing& r, int32_t T, const cs_traj_out& tr,
                              uint32_t seat_mask, int32_t* code, int32_t* pos, DevBuf& scan, hipStream_t s)
{
    const int64_t n = b.n, NP = n * r.P, M = NP + (int64_t)T * n;
    const int q4 = (r.O + 3) / 4;
    hipLaunchKernelGGL(k_replay_index, dim3((unsigned)((n + QBLOCK - 1) / QBLOCK)), dim3(QBLOCK), 0, s,
                       (const uint8_t*)tr.player, (const uint8_t*)tr.done, T, n, r.P, seat_mask, r.pvalid, code,
                       r.newpend);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipcub::TransformInputIterator<int32_t, ReplayCount, const int32_t*> counts(code, ReplayCount());
    if ((e = scan_sum(scan, counts, pos, (int)(M + 1), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_replay_write, dim3((unsigned)((M * q4 + QBLOCK - 1) / QBLOCK)), dim3(QBLOCK), 0, s, r, T, n,
                       (const uint8_t*)tr.obs, (const uint8_t*)tr.legal, (const uint8_t*)tr.player, tr.action,
                       (const float*)tr.reward, (const uint8_t*)tr.final_obs, code, pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_replay_carry, dim3((unsigned)((NP * q4 + QBLOCK - 1) / QBLOCK)), dim3(QBLOCK), 0, s, r, T, n,
                       (const uint8_t*)tr.obs, tr.action, code, pos);
    return hipGetLastError();
}

// idx[k] = the k-th oldest transition held: slot (total - size + idx[k]) % cap. One thread per (k, 4 obs units). An
// index outside [0, size) is the caller's error; it is clamped, so the kernel reads inside the ring whatever it is.
__global__ __launch_bounds__(QBLOCK) void k_replay_gather(ReplayRing r, const int64_t* __restrict__ idx, int64_t B,
                                                          float* o_st, int64_t* o_act, float* o_rew, float* o_nst,
                                                          uint8_t* o_nlg, uint8_t* o_dne)
{
    const int O = r.O;
    int64_t k;
    int c0;
    if (!row_col4((int64_t)blockIdx.x * QBLOCK + threadIdx.x, B, O, k, c0)) return;
    const int64_t total = *r.total, size = total < r.cap ? total : r.cap;
    const int64_t slot = (total - size + clamp_index(idx[k], size)) % r.cap;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (c0 + u < O) {
            if (o_st) o_st[k * O + c0 + u] = (float)r.st[slot * O + c0 + u];
            if (o_nst) o_nst[k * O + c0 + u] = (float)r.nst[slot * O + c0 + u];
        }
    }
    if (c0 == 0) {
        if (o_act) o_act[k] = r.act[slot];
        if (o_rew) o_rew[k] = r.rew[slot];
        if (o_dne) o_dne[k] = r.dne[slot];
        if (o_nlg)
            for (int u = 0; u < r.LB; u++) o_nlg[k * r.LB + u] = r.nlg[slot * r.LB + u];
    }
}

hipError_t launch_replay_gather(const ReplayRing& r, const int64_t* idx, int64_t B, const cs_replay_batch& o,
                                hipStream_t s)
{
    const int64_t work = B * ((r.O + 3) / 4);
    hipLaunchKernelGGL(k_replay_gather, dim3((unsigned)((work + QBLOCK - 1) / QBLOCK)), dim3(QBLOCK), 0, s, r, idx, B,
                       (float*)o.state, (int64_t*)o.action, (float*)o.reward, (float*)o.next_state,
                       (uint8_t*)o.next_legal, (uint8_t*)o.done);
    return hipGetLastError();
}

// ---- Double-DQN targets ----------------------------------------------------------------------------------------------
// best = first maximum of q_next over the legal actions (0 when none is legal: np.argmax of an all -inf row);
// target = reward + (done ? 0 : gamma) * q_next_target[best], the product and the sum each rounded to fp32.
__global__ __launch_bounds__(QBLOCK) void k_dqn_targets(const float* __restrict__ qn, const float* __restrict__ qt,
                                                        const uint8_t* __restrict__ next_legal,
                                                        const float* __restrict__ reward,
                                                        const uint8_t* __restrict__ done, int64_t B, int A, int LB,
                                                        float gamma, float* target, int32_t* best)
{
#pragma clang fp contract(off)   // the product and the sum below round separately (__fmul_rn / __fadd_rn are plain
                                 // operators in the headers' scope: under the default contraction the two fused)
    const int64_t i = (int64_t)blockIdx.x * QBLOCK + threadIdx.x;
    if (i >= B) return;
    int bi = -1;
    float bv = 0.f;
    for (int a = 0; a < A; a++) {
        if ((next_legal[i * LB + (a >> 3)] >> (a & 7)) & 1) {
            const float v = qn[i * A + a];
            if (bi < 0 || v > bv) {
                bi = a;
                bv = v;
            }
        }
    }
    if (bi < 0) bi = 0;
    if (best) best[i] = bi;
    if (target) {
        const float prod = (done[i] ? 0.f : gamma) * qt[i * A + bi];
        target[i] = reward[i] + prod;
    }
}

hipError_t launch_dqn_targets(const float* q_next, const float* q_next_target, const uint8_t* next_legal,
                              const float* reward, const uint8_t* done, int64_t B, int32_t A, float gamma,
                              float* target, int32_t* best, hipStream_t s)
{
    hipLaunchKernelGGL(k_dqn_targets, dim3((unsigned)((B + QBLOCK - 1) / QBLOCK)), dim3(QBLOCK), 0, s, q_next,
                       q_next_target, next_legal, reward, done, B, A, (A + 7) / 8, gamma, target, best);
    return hipGetLastError();
}

}  // namespace cs
