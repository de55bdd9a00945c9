// cs_dqn_train.hip -- the DQN learner on the device (rlcard/agents/dqn_agent.py train() and Estimator.update):
//
//   k_dqn_train       K dependent train steps in one launch of ONE workgroup of 1024 threads, nothing on the host in
//                     between. Per step: the batch's indices (given, or Floyd's sampling without replacement on Philox
//                     draws, by wave 0), the eval-mode forwards of next_state through the Q-network and the target
//                     network with k_dqn_targets' line, the train-mode forward of state (BatchNorm on the batch's
//                     statistics, the running statistics moved), the loss, the backward through the step's old weights
//                     and Adam on every parameter in place, then the copy into the target network where it is due.
//                     fp32 FMAs, every sum in a fixed order (no atomics, no order that scheduling decides): a step is
//                     a function of its inputs bit for bit, and K steps of one launch are K launches of one step.
//     layout          LDS holds, transposed [unit][row] with the rows padded to a multiple of 4 (BP): the batch's obs
//                     as the bytes the ring keeps (816 Mahjong bytes x 64 rows as floats would not fit), the BatchNorm
//                     vectors (mean, scale, shift, 1/std), the activations of every hidden layer (the backward needs
//                     them) and the output tile. The obs image shares its space with the activations of layers 1..:
//                     it is dead once layer 0 has read it, and it is gathered again from the ring where the next
//                     forward, or the first layer's backward, needs it (at most 52 KiB, from L2). The backward keeps
//                     no second set of buffers: delta_l overwrites h_l in place, element by element, which is why
//                     Adam is split -- first the gradient and the moments of W_{l+1} (they need h_l whole), then
//                     delta_l (it needs the OLD W_{l+1}), then the parameter update of W_{l+1} from the moments the
//                     same thread wrote. A weight's gradient never reaches memory (unless the debug output asks).
//                     The worst admitted case (816 obs bytes, 64 actions, B = 64, [128, 128, 128, 128]) takes
//                     163 072 B of the 163 840 a workgroup can have.
//     work split      forward: a thread per (output unit, 4 rows), the weights read as float4 along the input units
//                     (in input-unit order from the bias, like k_qnet); weight gradients: a thread per weight, its sum
//                     over the rows started at a row group that rotates with the input unit (LDS banks); deltas: a
//                     thread per (input unit, 4 rows); the first layer's backward: a thread per (obs column, group of
//                     output units), which also carries the column's share of the BatchNorm gradients -- with G[o][k]
//                     = sum_b delta_0[b][o] xhat[b][k]: dW_0[o][k] = gamma_k G + beta_k db_0[o], dgamma_k = sum_o
//                     W_0[o][k] G, dbeta_k = sum_o W_0[o][k] db_0[o]; the groups' partial sums meet in LDS in group
//                     order.
//     1024 threads    the phases are separated by 5 NH + 13 block barriers a step (NH hidden layers) and each offers
//                     out x rows / 4 .. out x in independent items: a Leduc [64, 64] step has 512 .. 4096 per phase, a
//                     [128, 128] one up to 30 720, each a dependent chain of 32 .. 816 FMAs fed from LDS and L1, so the
//                     step is latency-bound and wants every wave a CU can hold for one workgroup (16, four per SIMD,
//                     128 VGPRs each, which the kernel fits without scratch).
#include <math.h>
#include "cs_device.h"
#include "cs_dqn.h"

namespace cs {

constexpr int DT = 1024;      // threads of the workgroup
constexpr int DMAXB = 64;     // the largest batch: wave 0 holds a row per lane
constexpr int DMAXK = 4096;   // steps per launch
// per-row words of the batch at the start of LDS: slot i64, action, reward, done, y, err, best (4 B each), then the
// first layer's bias gradient f32 [128]
constexpr int DROWS_BYTES = DMAXB * 8 + 6 * DMAXB * 4 + CS_QNET_MAX_WIDTH * 4;

enum { DT_TANH = 0, DT_RELU = 1 };   // the hidden layers' activation
enum { DL_MSE = 0 };                 // the loss (NFSP's supervised step would add the cross-entropy)

struct TrainLds {
    int32_t BP;      // rows per unit: B rounded up to a multiple of 4
    int32_t NG;      // groups of output units in the first layer's backward (threads = NG * in_dim <= DT)
    int32_t o_bn, o_q, o_h0, o_r, o_part, bytes;   // byte offsets of the regions, and their total
};

static TrainLds train_layout(const cs_dqn_net& n, int B)
{
    TrainLds L;
    const int D = n.in_dim;
    L.BP = (B + 3) & ~3;
    L.NG = D < DT ? DT / D : 1;
    if (L.NG > n.hidden[0]) L.NG = n.hidden[0];
    int64_t o = DROWS_BYTES;
    L.o_bn = (int32_t)o;
    o += (int64_t)4 * D * 4;                                   // mean, scale, shift, 1/std
    L.o_q = (int32_t)o;
    o += (int64_t)n.num_actions * L.BP * 4;
    L.o_h0 = (int32_t)o;
    o += (int64_t)n.hidden[0] * L.BP * 4;
    L.o_r = (int32_t)o;
    int64_t obs = ((int64_t)D * L.BP + 15) & ~(int64_t)15, rest = 0;
    for (int l = 1; l < n.num_hidden; l++) rest += (int64_t)n.hidden[l] * L.BP * 4;
    o += obs > rest ? obs : rest;
    L.o_part = (int32_t)o;
    if (L.NG > 1) o += (int64_t)2 * L.NG * D * 4;
    L.bytes = (int32_t)o;
    return L;
}

int64_t dqn_train_lds_bytes(const cs_dqn_net& net, int32_t B)
{
    if (net.in_dim > DT) return INT64_MAX;   // (a thread per obs column in the first layer's backward)
    return train_layout(net, B).bytes;
}

struct AdamStep {
    float step, rbc2s, b1c, b2, b2c, eps;   // lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), 1 - beta1, beta2, 1 - beta2
};

__device__ __forceinline__ double pow_u64(double x, uint64_t n)
{
    double r = 1.0;
    while (n) {
        if (n & 1) r *= x;
        x *= x;
        n >>= 1;
    }
    return r;
}

__device__ __forceinline__ void adam_moments(const AdamStep& a, float g, float& m, float& v)
{
    m = m + a.b1c * (g - m);
    v = a.b2 * v + a.b2c * (g * g);
}

// six roundings: the two constants, sqrt, the FMA of the denominator, the product and the quotient
__device__ __forceinline__ float adam_param(const AdamStep& a, float p, float m, float v)
{
    return p - (a.step * m) / fmaf(sqrtf(v), a.rbc2s, a.eps);
}

__device__ __forceinline__ void adam_full(const AdamStep& a, float g, float* p, float* m, float* v)
{
    float m1 = *m, v1 = *v;
    adam_moments(a, g, m1, v1);
    *m = m1;
    *v = v1;
    *p = adam_param(a, *p, m1, v1);
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float x)
{
    if constexpr (ACT == DT_RELU) return fmaxf(x, 0.f);
    else return tanhf(x);
}

template <int ACT>
__device__ __forceinline__ float act_grad(float h)   // the activation's derivative from its output
{
    if constexpr (ACT == DT_RELU) return h > 0.f ? 1.f : 0.f;
    else return 1.f - h * h;
}

// cs_dqn_targets' line: the product and the sum round separately
__device__ __forceinline__ float dqn_target(float reward, bool done, float gamma, float qt)
{
#pragma clang fp contract(off)
    const float prod = (done ? 0.f : gamma) * qt;
    return reward + prod;
}

struct TrainCtx {
    int tid, B, BP, NBG, D, A, NH;
    int64_t* slot;
    int32_t *act, *dne, *best;
    float *rew, *y, *err, *db0;
    float *bnm, *bns, *bnb, *bnr;
    float *Q, *H0, *R, *part;
    uint8_t* xb;   // the obs image [D][BP] bytes, at R
};

// the batch's rows of src (the ring's state or next_state) -> xb [unit][row], the padding rows zero
__device__ __forceinline__ void train_gather(const TrainCtx& c, int O, const uint8_t* src)
{
    const int B = c.B, BP = c.BP;
    if ((O & 3) == 0) {   // (the ring's parts are 256-B aligned: whole dwords of a row)
        const int DG = O >> 2;
        for (int e = c.tid; e < B * DG; e += DT) {
            const int b = e / DG, u = e - b * DG;
            const uint32_t w = *(const uint32_t*)(src + c.slot[b] * O + 4 * u);
#pragma unroll
            for (int i = 0; i < 4; i++) c.xb[(4 * u + i) * BP + b] = (uint8_t)(w >> (8 * i));
        }
    } else {
        for (int e = c.tid; e < B * O; e += DT) {
            const int b = e / O, u = e - b * O;
            c.xb[u * BP + b] = src[c.slot[b] * O + u];
        }
    }
    const int pad = BP - B;
    for (int e = c.tid; e < pad * O; e += DT) {
        const int u = e / pad, b = B + (e - u * pad);
        c.xb[u * BP + b] = 0;
    }
}

// One Linear: xout[o][rows] = act(bias[o] + sum_k W[o][k] xin[k][rows]), a thread per (o, 4 rows), k ascending from the
// bias. BYTES: xin is the obs image and BatchNorm is applied on the way, (x - mean) * scale + shift.
template <int ACT, bool BYTES>
__device__ __forceinline__ void train_layer(const TrainCtx& c, const float* W, const float* bias, int in, int out,
                                            const void* xin, float* xout, bool act)
{
    const int BP = c.BP, NBG = c.NBG;
    const bool vec = (in & 3) == 0 && ((uintptr_t)W & 15) == 0;
#pragma unroll 1
    for (int it = c.tid; it < out * NBG; it += DT) {
        const int o = it / NBG, bg = it - o * NBG;
        const float* Wr = W + (int64_t)o * in;
        const float bo = bias[o];
        float a0 = bo, a1 = bo, a2 = bo, a3 = bo;
        auto mac = [&](int k, float w) {
            float x0, x1, x2, x3;
            if constexpr (BYTES) {
                const uint32_t x = *(const uint32_t*)((const uint8_t*)xin + k * BP + 4 * bg);
                const float m = c.bnm[k], s = c.bns[k], sh = c.bnb[k];
                x0 = fmaf((float)(x & 255u) - m, s, sh);
                x1 = fmaf((float)((x >> 8) & 255u) - m, s, sh);
                x2 = fmaf((float)((x >> 16) & 255u) - m, s, sh);
                x3 = fmaf((float)(x >> 24) - m, s, sh);
            } else {
                const float4 x = *(const float4*)((const float*)xin + k * BP + 4 * bg);
                x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
            }
            a0 = fmaf(w, x0, a0);
            a1 = fmaf(w, x1, a1);
            a2 = fmaf(w, x2, a2);
            a3 = fmaf(w, x3, a3);
        };
        if (vec) {
#pragma unroll 2
            for (int k = 0; k < in; k += 4) {
                const float4 w = *(const float4*)(Wr + k);
                mac(k, w.x);
                mac(k + 1, w.y);
                mac(k + 2, w.z);
                mac(k + 3, w.w);
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < in; k++) mac(k, Wr[k]);
        }
        if (act) {
            a0 = act_fwd<ACT>(a0);
            a1 = act_fwd<ACT>(a1);
            a2 = act_fwd<ACT>(a2);
            a3 = act_fwd<ACT>(a3);
        }
        *(float4*)(xout + o * BP + 4 * bg) = make_float4(a0, a1, a2, a3);
    }
}

// A forward of the batch's rows of src through net n -> c.Q [action][row], the hidden activations left in H0 and R.
// TRAIN: BatchNorm on the batch's statistics, which also move the running ones; otherwise on the running ones.
template <int ACT, bool TRAIN>
__device__ __forceinline__ void train_forward(const TrainCtx& c, int O, const cs_dqn_net& n, const uint8_t* src)
{
    const int B = c.B, BP = c.BP, D = c.D;
    train_gather(c, O, src);
    if constexpr (TRAIN) __syncthreads();
    for (int k = c.tid; k < D; k += DT) {
        if constexpr (TRAIN) {
            const uint8_t* col = c.xb + k * BP;
            int sum = 0;
            for (int b = 0; b < B; b++) sum += col[b];
            const float mean = (float)sum / (float)B;   // (the sum is exact)
            float ss = 0.f;
            for (int b = 0; b < B; b++) {
                const float d = (float)col[b] - mean;
                ss = fmaf(d, d, ss);
            }
            const float var = ss / (float)B, rstd = 1.0f / sqrtf(var + n.bn_eps), mom = n.bn_momentum;
            c.bnm[k] = mean;
            c.bnr[k] = rstd;
            c.bns[k] = n.bn_weight[k] * rstd;
            c.bnb[k] = n.bn_bias[k];
            n.bn_mean[k] = (1.0f - mom) * n.bn_mean[k] + mom * mean;
            n.bn_var[k] = (1.0f - mom) * n.bn_var[k] + mom * (ss / (float)(B - 1));
        } else {
            c.bnm[k] = n.bn_mean[k];
            c.bns[k] = n.bn_weight[k] / sqrtf(n.bn_var[k] + n.bn_eps);
            c.bnb[k] = n.bn_bias[k];
        }
    }
    if constexpr (TRAIN) {
        if (c.tid == 0) *n.bn_tracked += 1;
    }
    __syncthreads();
    train_layer<ACT, true>(c, n.W[0], n.b[0], D, n.hidden[0], c.xb, c.H0, true);
    __syncthreads();
    int in = n.hidden[0];
    const float* x = c.H0;
    float* nx = c.R;   // (layer 1's output lands on the obs image, dead by now)
    for (int l = 1; l < c.NH; l++) {
        const int out = n.hidden[l];
        train_layer<ACT, false>(c, n.W[l], n.b[l], in, out, x, nx, true);
        __syncthreads();
        x = nx;
        nx += out * BP;
        in = out;
    }
    train_layer<ACT, false>(c, n.W[c.NH], n.b[c.NH], in, c.A, x, c.Q, false);
    __syncthreads();
}

// offset of W[l] in the flat gradient vector (bn_weight, bn_bias, W[0], b[0], W[1], b[1], ...)
__device__ __forceinline__ int64_t grad_offset(const cs_dqn_net& n, int l)
{
    int64_t off = 2 * (int64_t)n.in_dim;
    int in = n.in_dim;
    for (int j = 0; j < l; j++) {
        off += (int64_t)n.hidden[j] * in + n.hidden[j];
        in = n.hidden[j];
    }
    return off;
}

template <int ACT, int LOSS>
__global__ __launch_bounds__(DT) void k_dqn_train(const ReplayRing r, const cs_dqn_net q, const cs_dqn_net tg,
                                                  const cs_dqn_adam opt, const cs_dqn_train_args a, const TrainLds L)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t t_lds[];
    static_assert(LOSS == DL_MSE, "the mean squared error is the one loss there is");
    const int tid0 = (int)threadIdx.x, B = a.B, K = a.K, D = q.in_dim, A = q.num_actions, NH = q.num_hidden;
    const int BP = L.BP, NBG = BP >> 2, O = r.O;
    TrainCtx c;
    c.B = B, c.BP = BP, c.NBG = NBG, c.D = D, c.A = A, c.NH = NH;
    c.slot = (int64_t*)t_lds;
    c.act = (int32_t*)(t_lds + DMAXB * 8);
    c.dne = c.act + DMAXB;
    c.best = c.dne + DMAXB;
    c.rew = (float*)(c.best + DMAXB);
    c.y = c.rew + DMAXB;
    c.err = c.y + DMAXB;
    c.db0 = c.err + DMAXB;
    c.bnm = (float*)(t_lds + L.o_bn);
    c.bns = c.bnm + D;
    c.bnb = c.bns + D;
    c.bnr = c.bnb + D;
    c.Q = (float*)(t_lds + L.o_q);
    c.H0 = (float*)(t_lds + L.o_h0);
    c.R = (float*)(t_lds + L.o_r);
    c.xb = t_lds + L.o_r;
    c.part = (float*)(t_lds + L.o_part);

    const int64_t total = *r.total, size = total < r.cap ? total : r.cap;
    if (!a.idx && size < B) {   // (every thread reads the same words: the workgroup leaves as one, before any barrier)
        for (int k = tid0; k < K; k += DT) a.loss[k] = NAN;
        return;
    }
    const int h0 = q.hidden[0];
    for (int k = 0; k < K; k++) {
        const uint64_t train_t = a.train_t0 + (uint64_t)k;
        // the thread's index, opaque to the optimizer once per step: what derives from it is formed where it is used,
        // not hoisted out of the step loop into registers that every phase then carries (the kernel has 128)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        c.tid = tid;
        // ---- the batch: wave 0, a row per lane -----------------------------------------------------------------------
        if (tid < WAVE) {
            int64_t pick = 0;
            if (a.idx) {
                if (tid < B) pick = clamp_index(a.idx[(int64_t)k * B + tid], size);
            } else {
                // Floyd: the i-th pick is r_i = floor(x_i (j + 1) / 2^64) with j = size - B + i, or j where r_i is
                // taken
                uint32_t w[4];
                philox4(a.seed, train_t, (uint64_t)tid, w);
                const uint64_t x = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                const long long mine = (long long)__umul64hi(x, (uint64_t)(size - B + tid + 1));
                for (int i = 0; i < B; i++) {
                    const long long ri = __shfl(mine, i);
                    const bool taken = __ballot(tid < i && pick == (int64_t)ri) != 0;
                    if (tid == i) pick = taken ? size - B + i : (int64_t)ri;
                }
            }
            if (tid < B) {
                const int64_t s = (total - size + pick) % r.cap;
                const int32_t ac = r.act[s];
                c.slot[tid] = s;
                c.act[tid] = ac < 0 ? 0 : (ac >= A ? A - 1 : ac);
                c.rew[tid] = r.rew[s];
                c.dne[tid] = r.dne[s];
                if (a.idx_out) a.idx_out[(int64_t)k * B + tid] = pick;
            }
        }
        __syncthreads();
        // ---- targets: eval forwards of next_state, then k_dqn_targets' line ------------------------------------------
        train_forward<ACT, false>(c, O, q, r.nst);
        if (tid < B) {   // (Q is next written by the target network's output layer, barriers away)
            const uint8_t* lg = r.nlg + c.slot[tid] * r.LB;
            int bi = -1;
            float bv = 0.f;
            for (int x = 0; x < A; x++) {
                if ((lg[x >> 3] >> (x & 7)) & 1) {
                    const float v = c.Q[x * BP + tid];
                    if (bi < 0 || v > bv) {
                        bi = x;
                        bv = v;
                    }
                }
            }
            c.best[tid] = bi < 0 ? 0 : bi;
        }
        train_forward<ACT, false>(c, O, tg, r.nst);
        if (tid < B) {
            const float y = dqn_target(c.rew[tid], c.dne[tid] != 0, a.gamma, c.Q[c.best[tid] * BP + tid]);
            c.y[tid] = y;
            if (a.target_out) a.target_out[(int64_t)k * B + tid] = y;
        }
        // ---- the train-mode forward of state, the loss and dL/dQ (in place of Q; zero on the padding rows) ----------
        train_forward<ACT, true>(c, O, q, r.st);
        if (tid < B) c.err[tid] = c.Q[c.act[tid] * BP + tid] - c.y[tid];
        __syncthreads();
        for (int it = tid; it < A * BP; it += DT) {
            const int x = it / BP, b = it - x * BP;
            c.Q[it] = (b < B && x == c.act[b]) ? 2.0f * c.err[b] / (float)B : 0.f;
        }
        if (tid == 0) {
            float s = 0.f;
            for (int b = 0; b < B; b++) s = fmaf(c.err[b], c.err[b], s);
            a.loss[k] = s / (float)B;
        }
        __syncthreads();
        // ---- Adam's constants of step t, the bias corrections in fp64 ------------------------------------------------
        AdamStep ad;
        {
            const uint64_t t = (uint64_t)opt.step0 + (uint64_t)k + 1;
            ad.step = (float)(opt.lr / (1.0 - pow_u64(opt.beta1, t)));
            ad.rbc2s = (float)(1.0 / sqrt(1.0 - pow_u64(opt.beta2, t)));
            ad.b1c = (float)(1.0 - opt.beta1);
            ad.b2 = (float)opt.beta2;
            ad.b2c = (float)(1.0 - opt.beta2);
            ad.eps = (float)opt.eps;
        }
        float* gout = (a.grads && k == K - 1) ? a.grads : nullptr;
        // ---- layers NH .. 1: X = delta of the layer's outputs [out][BP], Hp = its inputs' activations [in][BP] -------
        const float* X = c.Q;
        int out = A;
        for (int l = NH; l >= 1; l--) {
            const int in = q.hidden[l - 1];
            float* Hp = c.H0;
            if (l >= 2) {
                Hp = c.R;
                for (int j = 1; j < l - 1; j++) Hp += q.hidden[j] * BP;
            }
            float* W = q.W[l];
            float* Wm = opt.W_m[l];
            float* Wv = opt.W_v[l];
            const int64_t goff = gout ? grad_offset(q, l) : 0;
            // the gradient and the moments of W[l] (a thread per weight, the row groups rotated by the input unit)
            for (int it = tid; it < out * in; it += DT) {
                const int o = it / in, i = it - o * in;
                const float* dr = X + o * BP;
                const float* hr = Hp + i * BP;
                int gg = i % NBG;
                float g = 0.f;
                for (int s = 0; s < NBG; s++) {
                    const float4 d = *(const float4*)(dr + 4 * gg), h = *(const float4*)(hr + 4 * gg);
                    g = fmaf(d.x, h.x, g);
                    g = fmaf(d.y, h.y, g);
                    g = fmaf(d.z, h.z, g);
                    g = fmaf(d.w, h.w, g);
                    if (++gg == NBG) gg = 0;
                }
                float m = Wm[it], v = Wv[it];
                adam_moments(ad, g, m, v);
                Wm[it] = m;
                Wv[it] = v;
                if (gout) gout[goff + it] = g;
            }
            for (int o = tid; o < out; o += DT) {   // the bias (the backward does not read it): the whole update
                float g = 0.f;
                for (int b = 0; b < BP; b++) g += X[o * BP + b];
                adam_full(ad, g, q.b[l] + o, opt.b_m[l] + o, opt.b_v[l] + o);
                if (gout) gout[goff + (int64_t)out * in + o] = g;
            }
            __syncthreads();
            // delta of the inputs through the OLD W[l], in place of their activations (a thread per (i, 4 rows))
            for (int it = tid; it < in * NBG; it += DT) {
                const int i = it / NBG, bg = it - i * NBG;
                const float* Wc = W + i;
                float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;
                for (int o = 0; o < out; o++) {
                    const float w = Wc[(int64_t)o * in];
                    const float4 d = *(const float4*)(X + o * BP + 4 * bg);
                    u0 = fmaf(w, d.x, u0);
                    u1 = fmaf(w, d.y, u1);
                    u2 = fmaf(w, d.z, u2);
                    u3 = fmaf(w, d.w, u3);
                }
                float4* hp = (float4*)(Hp + i * BP + 4 * bg);
                const float4 h = *hp;
                *hp = make_float4(u0 * act_grad<ACT>(h.x), u1 * act_grad<ACT>(h.y), u2 * act_grad<ACT>(h.z),
                                  u3 * act_grad<ACT>(h.w));
            }
            __syncthreads();
            // W[l] from the moments this thread wrote above (nothing reads W[l] again in this step)
            for (int it = tid; it < out * in; it += DT) W[it] = adam_param(ad, W[it], Wm[it], Wv[it]);
            X = Hp;
            out = in;
        }
        // ---- layer 0: delta_0 is in H0; the obs image again (R is free: every delta above it has been consumed) ------
        train_gather(c, O, r.st);
        for (int o = tid; o < h0; o += DT) {
            float g = 0.f;
            for (int b = 0; b < BP; b++) g += c.H0[o * BP + b];
            c.db0[o] = g;
            adam_full(ad, g, q.b[0] + o, opt.b_m[0] + o, opt.b_v[0] + o);
            if (gout) gout[2 * (int64_t)D + (int64_t)h0 * D + o] = g;
        }
        __syncthreads();
        float pg = 0.f, pb = 0.f;   // this thread's share of dgamma_k, dbeta_k
        if (tid < L.NG * D) {
            const int og = tid / D, kk = tid - og * D;
            const float mean = c.bnm[kk], rstd = c.bnr[kk], gam = q.bn_weight[kk], bet = q.bn_bias[kk];
            const uint8_t* col = c.xb + kk * BP;
            for (int o = og; o < h0; o += L.NG) {
                const float* dr = c.H0 + o * BP;
                float G = 0.f;
                for (int s = 0; s < NBG; s++) {
                    const uint32_t x = *(const uint32_t*)(col + 4 * s);
                    const float4 d = *(const float4*)(dr + 4 * s);
                    G = fmaf(d.x, ((float)(x & 255u) - mean) * rstd, G);
                    G = fmaf(d.y, ((float)((x >> 8) & 255u) - mean) * rstd, G);
                    G = fmaf(d.z, ((float)((x >> 16) & 255u) - mean) * rstd, G);
                    G = fmaf(d.w, ((float)(x >> 24) - mean) * rstd, G);
                }
                const int64_t it = (int64_t)o * D + kk;
                const float dbo = c.db0[o], w = q.W[0][it];
                const float g = fmaf(gam, G, bet * dbo);
                pg = fmaf(w, G, pg);
                pb = fmaf(w, dbo, pb);
                adam_full(ad, g, q.W[0] + it, opt.W_m[0] + it, opt.W_v[0] + it);
                if (gout) gout[2 * (int64_t)D + it] = g;
            }
            if (L.NG > 1) {
                c.part[og * D + kk] = pg;
                c.part[(L.NG + og) * D + kk] = pb;
            }
        }
        __syncthreads();
        if (tid < D) {   // BatchNorm's weight and bias: the groups' shares in group order
            if (L.NG > 1) {
                pg = 0.f, pb = 0.f;
                for (int og = 0; og < L.NG; og++) {
                    pg += c.part[og * D + tid];
                    pb += c.part[(L.NG + og) * D + tid];
                }
            }
            adam_full(ad, pg, q.bn_weight + tid, opt.bn_weight_m + tid, opt.bn_weight_v + tid);
            adam_full(ad, pb, q.bn_bias + tid, opt.bn_bias_m + tid, opt.bn_bias_v + tid);
            if (gout) {
                gout[tid] = pg;
                gout[D + tid] = pb;
            }
        }
        __syncthreads();
        // ---- the target network follows, after the update, as train() has it ----------------------------------------
        if (a.target_every > 0 && train_t % (uint64_t)a.target_every == 0) {
            for (int i = tid; i < D; i += DT) {
                tg.bn_weight[i] = q.bn_weight[i];
                tg.bn_bias[i] = q.bn_bias[i];
                tg.bn_mean[i] = q.bn_mean[i];
                tg.bn_var[i] = q.bn_var[i];
            }
            if (tid == 0) *tg.bn_tracked = *q.bn_tracked;
            int in = D;
            for (int l = 0; l <= NH; l++) {
                const int o_n = l < NH ? q.hidden[l] : A;
                for (int i = tid; i < o_n * in; i += DT) tg.W[l][i] = q.W[l][i];
                for (int i = tid; i < o_n; i += DT) tg.b[l][i] = q.b[l][i];
                in = o_n;
            }
            __syncthreads();
        }
    }
}

hipError_t launch_dqn_train(const ReplayRing& r, const cs_dqn_net& qnet, const cs_dqn_net& target,
                            const cs_dqn_adam& opt, const cs_dqn_train_args& args, hipStream_t s)
{
    static_assert(DMAXK == 4096 && DMAXB == WAVE, "the ABI's ranges");
    const TrainLds L = train_layout(qnet, args.B);
    auto kern = k_dqn_train<DT_TANH, DL_MSE>;
    if (L.bytes > 65536) {   // past the default limit of dynamic LDS: raise this kernel's, as launch_net does
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, L.bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(1), dim3(DT), (size_t)L.bytes, s, r, qnet, target, opt, args, L);
    return hipGetLastError();
}

}  // namespace cs
