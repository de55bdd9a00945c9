// cs_skeleton.h -- the lockstep kernel skeleton shared by every lane-per-env game (one lane = one env, one wave = EPW
// consecutive envs): k_seed / k_reset / k_step / k_observe / k_rollout over a Game type (cs_leduc.h, cs_limit.h,
// cs_nolimit.h, cs_blackjack.h, cs_holdem_n.h), their host launchers and ops_of<G>, the game's launch table entry
// (cs_engine.h GameOps). Included by the translation units that instantiate games (cs_kernels.hip: the heads-up /
// single-table games; cs_holdem_n*.hip: 3..22-player hold'em).
// Integer/branchy work: no MFMA. The bound is HBM (obs/legal/reward rows out, packed state + RNG words in/out).
#pragma once
#include <cstddef>
#include <type_traits>

#include "cs_device.h"
#include "cs_ring.h"
#include "cs_engine.h"
#include "cs_dq.h"

namespace cs {

constexpr int BLOCK = 256;
constexpr int WAVES_PER_BLOCK = BLOCK / WAVE;

// a game's legal mask: one 64-bit word up to 64 actions, two up to 128 (cs_device.h Legal128), four up to 256 (Legal256)
template <class G>
using legal_t = std::conditional_t<(G::A > 128), Legal256, std::conditional_t<(G::A > 64), Legal128, uint64_t>>;

struct LaneCtx {
    int lane, wid;
    int64_t env, wave_first;
    int nvalid;
    bool valid;
};

// EPW envs per wave (lanes >= EPW idle): 64 everywhere but the rollouts of games with too few envs to fill the chip
// (Limit's 262 144 envs are 4 waves per SIMD at 64 per wave; half-full waves double that -- the step is latency-bound)
template <int EPW = WAVE>
__device__ __forceinline__ LaneCtx lane_ctx(int64_t n)
{
    LaneCtx c;
    c.lane = threadIdx.x & (WAVE - 1);
    c.wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);   // wave-uniform: wave_first lives in SGPRs
    const int64_t bx = (int64_t)blockIdx.x;   // plain block order (cs_device.h xcd_block measured slower for Leduc)
    c.wave_first = (bx * WAVES_PER_BLOCK + c.wid) * EPW;
    c.env = c.wave_first + c.lane;
    const int64_t left = n - c.wave_first;
    c.nvalid = left >= EPW ? EPW : (left > 0 ? (int)left : 0);
    c.valid = c.lane < EPW && c.env < n;
    return c;
}

// the lane-per-env games draw from the byte ring (cs_ring.h); invalid lanes get a ring that never needs a refill
template <int MODE = STAGE_NONE>
__device__ __forceinline__ RingLane<MODE> ring_lane(uint32_t* mt, const uint32_t* ctl, const LaneCtx& c)
{
    RingLane<MODE> m;
    if (c.valid) m.init(mt + c.env * RING_ENV_WORDS, ctl[c.env]);
    else m.init(mt, CTL_IDLE);
    return m;
}

// end-of-step refill (flag bit 0: skipped, every block crossing takes the in-lane serial path -- a test variant)
template <class M>
__device__ __forceinline__ void refill(M& m, int lane, int flags)
{
    if (!(flags & 1)) ring_refill_wave(m, lane);
}

// one 0/1 obs row from its bitmap as nontemporal 16-B stores by its own lane (G::OBS_DIRECT; rows are 16-B multiples,
// so a 16-B aligned tensor makes every store aligned; emit_obs falls back to dword stores for any other)
template <class G>
__device__ __forceinline__ void write_obs_rows16(uint8_t* o, const uint32_t (&bits)[G::NB])
{
    static_assert(!G::RAW_OBS && G::OBS % 16 == 0, "direct rows: 0/1 bytes, a 16-B multiple per row");
#pragma unroll
    for (int q = 0; q < G::OBS / 16; q++) {
        uint4 v;
        v.x = RowWriter<G::OBS>::expand4(bits[(4 * q) / 8] >> (4 * ((4 * q) % 8)));
        v.y = RowWriter<G::OBS>::expand4(bits[(4 * q + 1) / 8] >> (4 * ((4 * q + 1) % 8)));
        v.z = RowWriter<G::OBS>::expand4(bits[(4 * q + 2) / 8] >> (4 * ((4 * q + 2) % 8)));
        v.w = RowWriter<G::OBS>::expand4(bits[(4 * q + 3) / 8] >> (4 * ((4 * q + 3) % 8)));
        out_store16((uint4*)o + q, v);
    }
}

template <class G>
__device__ __forceinline__ void write_obs_direct(uint8_t* o, const uint32_t (&bits)[G::NB]);   // (below)

// The same for rows that are a dword multiple but no 16-B multiple (Gin Rummy's 260 B): row r starts at r * OBS, so the
// rows' 16-B phases differ and each lane decides for its own. H dwords (0..3) bring the address to a 16-B boundary,
// then nontemporal 16-B stores, then the dwords left over; a tensor that is not dword aligned takes byte stores.
template <class G, int H>
__device__ __forceinline__ void write_obs_row16_head(uint8_t* o, const uint32_t (&bits)[G::NB])
{
    constexpr int D = G::OBS / 4, Q = (D - H) / 4;
    auto dword = [&](int j) { return RowWriter<G::OBS>::expand4(bits[j / 8] >> (4 * (j % 8))); };
#pragma unroll
    for (int j = 0; j < H; j++) out_store((uint32_t*)o + j, dword(j));
#pragma unroll
    for (int q = 0; q < Q; q++) {
        uint4 v;
        v.x = dword(H + 4 * q);
        v.y = dword(H + 4 * q + 1);
        v.z = dword(H + 4 * q + 2);
        v.w = dword(H + 4 * q + 3);
        out_store16((uint4*)((uint32_t*)o + H) + q, v);
    }
#pragma unroll
    for (int j = H + 4 * Q; j < D; j++) out_store((uint32_t*)o + j, dword(j));
}
template <class G>
__device__ __forceinline__ void write_obs_rows16_any(uint8_t* o, const uint32_t (&bits)[G::NB])
{
    static_assert(!G::RAW_OBS && G::OBS % 4 == 0 && G::OBS >= 32, "direct rows: 0/1 bytes, a dword multiple per row");
    const uint32_t a = (uint32_t)(uintptr_t)o & 15u;
    if (a == 0u) write_obs_row16_head<G, 0>(o, bits);
    else if (a == 12u) write_obs_row16_head<G, 1>(o, bits);
    else if (a == 8u) write_obs_row16_head<G, 2>(o, bits);
    else if (a == 4u) write_obs_row16_head<G, 3>(o, bits);
    else {
#pragma unroll 4
        for (int k = 0; k < G::OBS; k++) o[k] = (uint8_t)((bits[k >> 5] >> (k & 31)) & 1u);
    }
}

// Rows of any length that hold a raw-byte field among their 0/1 bytes (G::RAW_SPAN_LEN > 0, Bridge's 573 B): row r
// starts at r * OBS, so a wave's lanes see every byte phase and every 16-B phase, and a row shares a 16-B piece with its
// neighbour at both ends: a lane stores its own bytes only. mixed_dword is dword j of the row's value stream (bytes 4 j
// .. 4 j + 3; zero past the row), j a constant after unrolling, so no bitmap word is indexed dynamically.
template <class G>
__device__ __forceinline__ uint32_t mixed_dword(const uint32_t (&bits)[G::NB], int j)
{
    constexpr int ND = (G::OBS + 3) / 4;
    static_assert(ND <= 8 * G::NBITS && G::NB == G::NBITS + G::RAW_SPAN_LEN / 4 && G::RAW_SPAN_LEN % 4 == 0 &&
                      G::RAW_SPAN_AT + G::RAW_SPAN_LEN <= G::OBS,
                  "mixed rows: the bitmap words, then the span's bytes");
    if (j >= ND) return 0u;
    uint32_t v = RowWriter<4>::expand4(bits[j / 8] >> (4 * (j % 8)));
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int sb = 4 * j + i - G::RAW_SPAN_AT;   // this byte's place in the span
        if (sb >= 0 && sb < G::RAW_SPAN_LEN) v |= ((bits[G::NBITS + sb / 4] >> (8 * (sb % 4))) & 255u) << (8 * i);
    }
    return v;
}
// The row from its first dword-aligned byte on: hb (0..3) bytes before it were stored by the caller, so stream dword i
// is alignbyte(dword i + 1, dword i, hb), one more VALU instruction per dword. H dwords (0..3, a template argument: the
// indices stay constants) bring the address to a 16-B boundary, then 16-B stores, then the dwords and bytes left over:
// (OBS - hb) / 4 whole dwords, NDMIN or one more, and at most three bytes.
// The stores are plain, not nontemporal: neighbouring rows share cache lines at both ends and a lane's 16-B pieces are
// 573 B apart from the next lane's, so the lines fill up in L2 over many instructions; streamed past the caches the same
// stores measured about six times slower (profiles/EXPERIMENTS.md B-1; cs_prof.h CS_PROF_MIXED_NT).
template <class T>
__device__ __forceinline__ void mixed_store(T* p, T v)
{
#if CS_PROF_MIXED_NT
    out_store(p, v);
#else
    *p = v;
#endif
}
__device__ __forceinline__ void mixed_store16(uint4* p, const uint4& v)
{
#if CS_PROF_MIXED_NT
    out_store16(p, v);
#else
    *p = v;
#endif
}
template <class G, int H>
__device__ __forceinline__ void write_obs_mixed_head(uint8_t* o, const uint32_t (&bits)[G::NB], uint32_t hb)
{
    constexpr int NDMIN = (G::OBS - 3) / 4, Q = (NDMIN - H) / 4;
    uint32_t* od = (uint32_t*)(o + hb);
    uint32_t lo = mixed_dword<G>(bits, 0);
    auto next = [&](int i) {
        const uint32_t hi = mixed_dword<G>(bits, i + 1);
        const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, hb);
        lo = hi;
        return v;
    };
#pragma unroll
    for (int j = 0; j < H; j++) mixed_store(od + j, next(j));
#pragma unroll
    for (int q = 0; q < Q; q++) {
        uint4 v;
        v.x = next(H + 4 * q);
        v.y = next(H + 4 * q + 1);
        v.z = next(H + 4 * q + 2);
        v.w = next(H + 4 * q + 3);
        mixed_store16((uint4*)(od + H) + q, v);
    }
#pragma unroll
    for (int j = H + 4 * Q; j < NDMIN; j++) mixed_store(od + j, next(j));
    const uint32_t sa = next(NDMIN), sb = next(NDMIN + 1);
    const uint32_t nd = ((uint32_t)G::OBS - hb) >> 2, tb = (uint32_t)G::OBS - hb - 4u * nd;
    const bool more = nd > (uint32_t)NDMIN;
    if (more) mixed_store(od + NDMIN, sa);
    const uint32_t tail = more ? sb : sa;
    uint8_t* ot = (uint8_t*)(od + nd);
    if (tb > 0u) mixed_store(ot, (uint8_t)tail);
    if (tb > 1u) mixed_store(ot + 1, (uint8_t)(tail >> 8));
    if (tb > 2u) mixed_store(ot + 2, (uint8_t)(tail >> 16));
}
// Mixed rows that are a 16-B multiple (Scout's 688 B): the row stride keeps the tensor's alignment, so an aligned tensor
// takes OBS / 16 whole 16-B stores per row and none of the phase work above. Plain stores, as for the rows above: a
// lane's pieces are 688 B apart from the next lane's, and streamed past the caches they measured 5.7 times slower
// (profiles/EXPERIMENTS.md SC-1; cs_prof.h CS_PROF_MIXED16_NT)
template <class G>
__device__ __forceinline__ void write_obs_mixed16(uint8_t* o, const uint32_t (&bits)[G::NB])
{
    static_assert(G::RAW_SPAN_LEN > 0 && G::OBS % 16 == 0, "mixed rows of whole 16-B pieces");
#pragma unroll
    for (int q = 0; q < G::OBS / 16; q++) {
        uint4 v;
        v.x = mixed_dword<G>(bits, 4 * q);
        v.y = mixed_dword<G>(bits, 4 * q + 1);
        v.z = mixed_dword<G>(bits, 4 * q + 2);
        v.w = mixed_dword<G>(bits, 4 * q + 3);
#if CS_PROF_MIXED16_NT
        out_store16((uint4*)o + q, v);
#else
        *((uint4*)o + q) = v;
#endif
    }
}
template <class G>
__device__ __forceinline__ void write_obs_mixed(uint8_t* o, const uint32_t (&bits)[G::NB])
{
#if CS_PROF_MIXED_WRITER == 1   // A/B: the row as a byte loop, which the compiler merges into unaligned wide stores
    write_obs_direct<G>(o, bits);
#else
    const uint32_t hb = (0u - (uint32_t)(uintptr_t)o) & 3u;   // bytes up to the first dword boundary
    const uint32_t d0 = mixed_dword<G>(bits, 0);
    if (hb > 0u) mixed_store(o, (uint8_t)d0);
    if (hb > 1u) mixed_store(o + 1, (uint8_t)(d0 >> 8));
    if (hb > 2u) mixed_store(o + 2, (uint8_t)(d0 >> 16));
    const uint32_t a = (uint32_t)(uintptr_t)(o + hb) & 15u;
    if (a == 0u) write_obs_mixed_head<G, 0>(o, bits, hb);
    else if (a == 12u) write_obs_mixed_head<G, 1>(o, bits, hb);
    else if (a == 8u) write_obs_mixed_head<G, 2>(o, bits, hb);
    else write_obs_mixed_head<G, 3>(o, bits, hb);
#endif
}

// obs rows: staged + coalesced when the row is a dword multiple, per-lane bytes otherwise
template <class G, int ROWS = WAVE>
__device__ __forceinline__ void emit_obs(uint32_t* lds, const uint32_t (&bits)[G::NB], uint8_t* obs, int64_t row0, int flags,
                                         const LaneCtx& c)
{
    if constexpr (G::RAW_SPAN_LEN > 0 && G::OBS % 16 == 0) {
        static_assert(G::OBS_DIRECT && !G::RAW_OBS, "mixed rows are stored by their own lane");
        if (c.valid) write_obs_direct<G>(obs + (row0 + c.lane) * G::OBS, bits);   // (16-B pieces on an aligned tensor)
    } else if constexpr (G::RAW_SPAN_LEN > 0) {
        static_assert(G::OBS_DIRECT && !G::RAW_OBS && G::OBS >= 32, "mixed rows are stored by their own lane");
        if (c.valid) write_obs_mixed<G>(obs + (row0 + c.lane) * G::OBS, bits);
    } else if constexpr (G::OBS_DIRECT && G::OBS % 16 != 0) {
        if (c.valid) write_obs_rows16_any<G>(obs + (row0 + c.lane) * G::OBS, bits);   // (decided per row)
    } else if constexpr (G::OBS_DIRECT) {
        if (c.valid) {   // (the row stride is a 16-B multiple: the tensor's alignment is every row's)
            uint8_t* o = obs + (row0 + c.lane) * G::OBS;
            if ((((uintptr_t)o) & 15u) == 0) write_obs_rows16<G>(o, bits);
            else write_obs_direct<G>(o, bits);
        }
    } else if constexpr (G::RAW_OBS && G::OBS % 2 == 0) {
        RowWriterRaw<G::OBS, ROWS>::write(lds, bits, obs + row0 * G::OBS, c.lane, c.nvalid, !(flags & 4));
    } else if constexpr (G::RAW_OBS) {
        if (c.valid) {
            uint8_t* o = obs + (row0 + c.lane) * G::OBS;
#pragma unroll
            for (int k = 0; k < G::OBS; k++) o[k] = (uint8_t)(bits[k >> 2] >> (8 * (k & 3)));
        }
    } else if constexpr (G::OBS % 4 == 0) {
        RowWriter<G::OBS, ROWS>::write(lds, bits, obs + row0 * G::OBS, c.lane, c.nvalid, !(flags & 4));
    } else {
        if (c.valid) {
            uint8_t* o = obs + (row0 + c.lane) * G::OBS;
#pragma unroll
            for (int k = 0; k < G::OBS; k++) o[k] = (uint8_t)((bits[k >> 5] >> (k & 31)) & 1u);
        }
    }
}

// one obs row straight from a lane (final observations: only the lanes whose game just ended write)
template <class G>
__device__ __forceinline__ void write_obs_direct(uint8_t* o, const uint32_t (&bits)[G::NB])
{
    if constexpr (G::RAW_SPAN_LEN > 0) {   // (mixed rows, any alignment: a byte loop; the compiler merges neighbours)
        if constexpr (G::OBS % 16 == 0) {
            if ((((uintptr_t)o) & 15u) == 0) {
                write_obs_mixed16<G>(o, bits);
                return;
            }
        }
#pragma unroll
        for (int j = 0; j < (G::OBS + 3) / 4; j++) {
            const uint32_t v = mixed_dword<G>(bits, j);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (4 * j + i < G::OBS) o[4 * j + i] = (uint8_t)(v >> (8 * i));
            }
        }
    } else if constexpr (G::RAW_OBS) {
#pragma unroll
        for (int k = 0; k < G::OBS; k++) o[k] = (uint8_t)(bits[k >> 2] >> (8 * (k & 3)));
    } else if constexpr (G::OBS % 4 == 0) {
#pragma unroll
        for (int j = 0; j < G::OBS / 4; j++)
            ((uint32_t*)o)[j] = RowWriter<G::OBS>::expand4(bits[j / 8] >> (4 * (j % 8)));
    } else {
#pragma unroll
        for (int k = 0; k < G::OBS; k++) o[k] = (uint8_t)((bits[k >> 5] >> (k & 31)) & 1u);
    }
}

template <class G>
__device__ __forceinline__ void emit_legal(uint8_t* legal, int64_t row, uint64_t lg)
{
#pragma unroll
    for (int k = 0; k < G::LB; k++) out_store(legal + row * G::LB + k, (uint8_t)(lg >> (8 * k)));
}

template <class G>
__device__ __forceinline__ void emit_legal(uint8_t* legal, int64_t row, const Legal128& lg)
{
    static_assert(G::LB > 8 && G::LB <= 16, "two-word legal rows");
#pragma unroll
    for (int k = 0; k < 8; k++) out_store(legal + row * G::LB + k, (uint8_t)(lg.lo >> (8 * k)));
#pragma unroll
    for (int k = 8; k < G::LB; k++) out_store(legal + row * G::LB + k, (uint8_t)(lg.hi >> (8 * (k - 8))));
}

template <class G>
__device__ __forceinline__ void emit_legal(uint8_t* legal, int64_t row, const Legal256& lg)
{
    static_assert(G::LB > 16 && G::LB <= 32, "four-word legal rows");
#pragma unroll
    for (int k = 0; k < G::LB; k++) out_store(legal + row * G::LB + k, (uint8_t)(lg.w[k / 8] >> (8 * (k % 8))));
}

template <class G>
__device__ __forceinline__ void emit_reward(float* reward, int64_t row, const float (&r)[G::P])
{
    if constexpr (G::P == 2) {
        uint64_t v = (uint64_t)__float_as_uint(r[0]) | (uint64_t)__float_as_uint(r[1]) << 32;
        if constexpr (G::REWARD_OPAQUE) asm volatile("" : "+v"(v));
        out_store((uint64_t*)(reward + row * 2), v);
    } else {
#pragma unroll
        for (int k = 0; k < G::P; k++) reward[row * G::P + k] = r[k];
    }
}

// LDS words of a wave's obs span image: bit rows (RowWriter, dword multiples), raw byte rows (RowWriterRaw, even)
template <class G, int ROWS>
constexpr int obs_lds_words()
{
    if constexpr (G::OBS_DIRECT) return 1;
    else if constexpr (!G::RAW_OBS && G::OBS % 4 == 0) return RowWriter<G::OBS, ROWS>::LDS_WORDS;
    else if constexpr (G::RAW_OBS && G::OBS % 2 == 0) return RowWriterRaw<G::OBS, ROWS>::LDS_WORDS;
    else return 1;
}
template <class G, int ROWS = WAVE>
struct ObsLds {
    static constexpr int WORDS = obs_lds_words<G, ROWS>();
};
template <class G>
struct StageBytes {   // a wave's staged rows in the rollout's LDS
    static constexpr int value = Stage<G::STAGE_W, G::STAGE_PAD, G::EPW>::BYTES;
    // the staged-byte scans read one dword past their last staged byte (RingLane::interval, draw_intervals)
    static_assert(G::STAGE_PAD >= 4, "stage rows need a pad of at least a dword");
};
// restage after the refill: STAGE_R starts one, STAGE_RF (>= STAGE_R) picks the lanes it takes (ring_restage_wave)
template <class G>
__device__ __forceinline__ void restage(RingLane<STAGE_LDS>& m, uint8_t* area, int lane, bool valid)
{
    ring_restage_wave<G::STAGE_W, G::STAGE_PAD, G::STAGE_R, G::RESTAGE_B, G::STAGE_RF>(m, area, lane, valid);
}
template <class G>
struct Scratch {   // per-lane LDS words of games that keep state in LDS (blackjack); one word per wave otherwise
    static constexpr int WORDS = G::SCRATCH_WORDS > 0 ? G::SCRATCH_WORDS * WAVE : 1;
};
template <class G>
__device__ __forceinline__ uint32_t* scratch_of(uint32_t* wave_area, int lane)
{
    return G::SCRATCH_WORDS > 0 ? wave_area + lane : nullptr;
}
// Env.get_payoffs at the step that ends the game (PAYOFF_DRAWS: the judge takes the lane's RNG)
template <class G, class Rng>
__device__ __forceinline__ void game_payoffs(G& g, float (&r)[G::P], Rng& rng)
{
    if constexpr (G::PAYOFF_DRAWS) g.payoffs(r, rng);
    else g.payoffs(r);
}

// Game.init_game for k_reset / k_step. A forwarding layer only, and kept: with game_reset_hbm called directly the
// compiler orders a few operands of k_reset<Nolimit> and k_step<Nolimit> differently (same instructions and registers)
template <class G, class Rng>
__device__ __forceinline__ void game_reset(G& g, Rng& rng, uint32_t* st, int64_t n, int64_t env)
{
    game_reset_hbm(g, rng, st, n, env);
}

// StepRecord (cs_engine.h): the wave holding env rec.env writes its state words and, after a system-scope fence (it
// waits for every store the wave issued: its obs rows, legal bytes, player, reward, done), the sequence number
template <class G>
__device__ __forceinline__ void step_record(const StepRecord& rec, const uint32_t* st, int64_t n, const LaneCtx& c)
{
    if (rec.seq == nullptr || rec.env < c.wave_first || rec.env >= c.wave_first + WAVE) return;   // wave-uniform
    if (c.valid && c.env == rec.env) {
#pragma unroll
        for (int w = 0; w < G::WORDS; w++) rec.words[w] = st[(int64_t)w * n + c.env];
    }
    __threadfence_system();
    if (c.valid && c.env == rec.env) __hip_atomic_store(rec.seq, rec.seqv, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

#define CS_SMEM_ROWS(G, ROWS)                                         \
    __shared__ uint32_t lds[WAVES_PER_BLOCK][ObsLds<G, ROWS>::WORDS]; \
    __shared__ uint32_t scr[WAVES_PER_BLOCK][Scratch<G>::WORDS]
#define CS_SMEM(G) CS_SMEM_ROWS(G, WAVE)

// ------------------------------------------------------------------------------------------------------------------
// Seeding, a lane per env (env first + i takes key i): S0 = init_by_array(key) in wbuf, then the env's first blocks
// generated in place, and a finished game, so the next reset / step deals
template <class G>
__global__ __launch_bounds__(BLOCK) void k_seed(uint32_t* mt, uint32_t* ctl, uint32_t* st, int64_t n,
                                                 const uint32_t* keys, const int32_t* klen, int64_t first,
                                                 int64_t count, int /* kernel flags: none applies */, GameParams prm)
{
    __shared__ uint32_t scr[WAVES_PER_BLOCK][Scratch<G>::WORDS];
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    const int64_t env = first + i;
    uint32_t* wbuf = mt + env * RING_ENV_WORDS;
    const int kl = klen[i] == 2 ? 2 : 1;                    // validated on the host; never trust it here
    const uint32_t phx = prm.rng_mode == CS_RNG_PHILOX ? CTL_PHILOX : 0u;
    const uint32_t kb = seed_blocks(env);                  // blocks 0..kb-1 now (cs_ring.h seed_blocks)
    if (phx) {   // Philox byte stream: key = the init_by_array key, blocks 0..kb-1 into slots 0..kb-1, counter kb
        wbuf[0] = 0u;
        wbuf[1] = keys[2 * i];
        wbuf[2] = kl == 2 ? keys[2 * i + 1] : 0u;
        ring_gen_philox((gu32*)wbuf, SLOT_MASK, 0, 1, (int)kb);
        wbuf[0] = kb;
    } else {
        mt_init_by_array(wbuf, keys + 2 * i, kl);
        for (uint32_t b = 0; b < kb; b++) {     // numpy's first draws: block 0 = twist(S0)
            mt_twist_inplace(wbuf);
            ring_bytes_serial(wbuf, (uint8_t*)(wbuf + MT_N), b);
        }
    }
    G g;
    g.bind(scratch_of<G>(scr[threadIdx.x / WAVE], lane), prm);
    g.blank();
    g.store(st, n, env);
    if constexpr (DqOf<G>::value > 0) st[(int64_t)G::GW * n + env] = 0u;   // empty deal queue
    ctl[env] = 0u | (kb - 1u) << CTL_LAT_SHIFT | phx;   // position 0, latest block in slot kb - 1
}

template <class G>
__global__ __launch_bounds__(BLOCK) void k_reset(uint32_t* mt, uint32_t* ctl, uint32_t* st, int64_t n,
                                                  cs_step_out out, int flags, GameParams prm, StepRecord rec)
{
    CS_SMEM(G);
    const LaneCtx c = lane_ctx(n);
    RingLane<> m = ring_lane(mt, ctl, c);
    G g;
    g.bind(scratch_of<G>(scr[c.wid], c.lane), prm);
    g.blank();
    if (c.valid) {
        g.load(st, n, c.env);   // the Game object outlives init_game (limit-holdem's raise history, :98/:101)
        game_reset(g, m, st, n, c.env);
    }
    refill(m, c.lane, flags & 1);
    uint32_t bits[G::NB];
    const int p = g.current();
    g.observe(p, bits);
    if (out.obs) emit_obs<G>(lds[c.wid], bits, (uint8_t*)out.obs, c.wave_first, flags, c);
    if (c.valid) {
        if (out.legal) emit_legal<G>((uint8_t*)out.legal, c.env, g.legal());
        if (out.player) ((uint8_t*)out.player)[c.env] = (uint8_t)p;
        if (out.reward) {
            float r[G::P];
#pragma unroll
            for (int k = 0; k < G::P; k++) r[k] = 0.f;
            emit_reward<G>((float*)out.reward, c.env, r);
        }
        if (out.done) ((uint8_t*)out.done)[c.env] = (uint8_t)g.is_over();
        g.store(st, n, c.env);
        ctl[c.env] = m.ctl_word();
    }
    step_record<G>(rec, st, n, c);
}

template <class G>
__global__ __launch_bounds__(BLOCK) void k_step(uint32_t* mt, uint32_t* ctl, uint32_t* st, int64_t n,
                                                 const int32_t* actions, cs_step_out out, int flags,
                                                 GameParams prm, StepRecord rec)
{
    CS_SMEM(G);
    const LaneCtx c = lane_ctx(n);
    RingLane<> m = ring_lane(mt, ctl, c);
    G g;
    g.bind(scratch_of<G>(scr[c.wid], c.lane), prm);
    g.blank();
    float r[G::P];
#pragma unroll
    for (int k = 0; k < G::P; k++) r[k] = 0.f;
    bool done = false;
    if (c.valid) {
        g.load(st, n, c.env);
        if (g.is_over()) {
            game_reset(g, m, st, n, c.env);
        } else {
            g.step(actions[c.env], m);
            done = g.is_over();
            if (done) game_payoffs(g, r, m);
        }
    }
    refill(m, c.lane, flags & 1);
    uint32_t bits[G::NB];
    const int p = g.current();
    g.observe(p, bits);
    if (out.obs) emit_obs<G>(lds[c.wid], bits, (uint8_t*)out.obs, c.wave_first, flags, c);
    if (c.valid) {
        if (out.legal) emit_legal<G>((uint8_t*)out.legal, c.env, g.legal());
        if (out.player) ((uint8_t*)out.player)[c.env] = (uint8_t)p;
        if (out.reward) emit_reward<G>((float*)out.reward, c.env, r);
        if (out.done) ((uint8_t*)out.done)[c.env] = (uint8_t)done;
        g.store(st, n, c.env);
        ctl[c.env] = m.ctl_word();
    }
    step_record<G>(rec, st, n, c);
}

template <class G>
__global__ __launch_bounds__(BLOCK) void k_observe(const uint32_t* st, int64_t n, int player, cs_step_out out,
                                                    GameParams prm, StepRecord rec)
{
    CS_SMEM(G);
    const LaneCtx c = lane_ctx(n);
    G g;
    g.bind(scratch_of<G>(scr[c.wid], c.lane), prm);
    g.blank();
    if (c.valid) g.load(st, n, c.env);
    uint32_t bits[G::NB];
    g.observe(player, bits);
    if (out.obs) emit_obs<G>(lds[c.wid], bits, (uint8_t*)out.obs, c.wave_first, 0, c);
    if (c.valid) {
        if (out.legal) emit_legal<G>((uint8_t*)out.legal, c.env, g.legal());
        if (out.player) ((uint8_t*)out.player)[c.env] = (uint8_t)g.current();
        if (out.done) ((uint8_t*)out.done)[c.env] = (uint8_t)g.is_over();
    }
    step_record<G>(rec, st, n, c);
}

// k_rollout's arguments as one struct, read from the kernarg segment through a pointer that every step makes opaque
// again (RolloutArgsK): the loop's uses (outputs, policy key, flags) are scalar loads where the step needs them instead
// of SGPRs live for the whole kernel, which the compiler spilled to VGPR lanes and restored with v_readlane (a VALU
// instruction) at every use (ddz::PairArgs, the same for DouDizhu)
struct RolloutArgs {
    uint32_t* mt;
    uint32_t* ctl;
    uint32_t* st;
    int64_t n;
    uint64_t seed, t0, env_base;
    cs_traj_out out;
    GameParams prm;
    uint32_t* sctl;
    uint8_t* sbuf;
    int32_t T, flags;
    uint32_t seats;   // k_rollout<G, true>: byte p = seat p's CS_POLICY_* id (one scalar word for the per-step choice)
    uint32_t pad_;
};
typedef const __attribute__((address_space(4))) RolloutArgs* RolloutArgsK;
// k_rollout (either instantiation) reads its argument back through __builtin_amdgcn_kernarg_segment_ptr(), so
// RolloutArgs must stay the kernel's ONLY explicit parameter (then it sits at kernarg offset 0 with exactly the host
// layout): any new argument goes inside the struct
static_assert(std::is_standard_layout<RolloutArgs>::value && std::is_trivially_copyable<RolloutArgs>::value,
              "RolloutArgs is copied into the kernarg segment bytewise");
static_assert(offsetof(RolloutArgs, mt) == 0 && alignof(RolloutArgs) == 8 && sizeof(RolloutArgs) % 8 == 0,
              "RolloutArgs: first kernarg at offset 0, 8-byte aligned");

// The rollout. POL = false (cs_rollout) plays the uniform-random policy; POL = true (cs_rollout_policy) is a second
// instantiation in which seat p plays byte p of args.seats (CS_POLICY_*). Everything the policy path adds sits inside
// `if constexpr (POL)`, so the random rollout -- tuned to its register budget, see the comments below -- compiles from
// the same statements as before the policy path existed.
template <class G, bool POL = false>
__global__ __launch_bounds__(BLOCK, G::MIN_WAVES) void k_rollout(RolloutArgs args)
{
    RolloutArgsK ak = (RolloutArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    auto arg = [&]() -> const RolloutArgs& {
        asm volatile("" : "+s"(ak));
        return *(const RolloutArgs*)ak;
    };
    uint32_t* const mt = args.mt;
    uint32_t* const ctl = args.ctl;
    uint32_t* const st = args.st;
    const int64_t n = args.n;
    const int T = args.T, flags = args.flags;
    const GameParams prm = args.prm;
    uint32_t* const sctl = args.sctl;
    uint8_t* const sbuf = args.sbuf;
    CS_SMEM_ROWS(G, G::EPW);
    __shared__ __attribute__((aligned(16))) uint8_t stage[WAVES_PER_BLOCK][StageBytes<G>::value];
    const LaneCtx c = lane_ctx<G::EPW>(n);
    RingLane<STAGE_LDS> m = ring_lane<STAGE_LDS>(mt, ctl, c);
    // MT staging needs both blocks valid at every restage, i.e. the cooperative refill (flag bit 0 off);
    // flag bit 1 disables it (one global load per draw) for A/B runs and fallback-path tests
    const bool staged = !(flags & 3);
    // the staged rows left by the previous launch stay valid while ctl bit 17 is set (single-step kernels and
    // seeding rewrite ctl without it)
    uint8_t* rows = sbuf + c.wave_first * G::STAGE_W;
    if (staged) {
        if (c.valid && ((ctl[c.env] >> 17) & 1u)) {
            const uint32_t w = sctl[c.env];
            m.sp = w & 0xFFFFu;
            m.sn = w >> 16;
        }
        stage_rows_copy<G::STAGE_W, G::STAGE_PAD>(stage[c.wid], rows, c.lane, c.nvalid, true);
    }
    // the deal queues of the wave's envs for the launch in LDS (DQW consecutive words per lane: odd stride)
    constexpr int DQ = DqOf<G>::value, DQW = DqOf<G>::words;
    __shared__ uint32_t dql[DQ > 0 ? WAVES_PER_BLOCK * G::EPW * DQW : 1];
    DqMem q{};
    if constexpr (DQ > 0) {
        q = DqMem{dql + (c.wid * G::EPW + (c.lane < G::EPW ? c.lane : 0)) * DQW, 1};
        if (c.valid) {
#pragma unroll
            for (int w = 0; w < DQW; w++) q.set(w, st[(int64_t)(G::GW + w) * n + c.env]);
        }
    }
    G g;
    g.bind(scratch_of<G>(scr[c.wid], c.lane), prm);
    g.blank();
    if (c.valid) {
        g.load(st, n, c.env);
        if (g.is_over()) {
            if constexpr (DQ > 0) dq_reset(g, m, q);
            else g.reset(m);
        }
    }
    refill(m, c.lane, flags & 1);
    if (staged) restage<G>(m, stage[c.wid], c.lane, c.valid);
    PolicyRng pol;
    const uint64_t genv0 = args.env_base + (uint64_t)c.env;   // the policy counter's env id
    for (int t = 0; t < T; t++) {
        const RolloutArgs& A = arg();
        // the lane id made opaque at every step, so lane-derived values (env id, row and LDS addresses) are recomputed
        // from it instead of held across the step -- at 6 waves per SIMD (80 VGPRs) the held copies were spilled, and
        // a spill reload waits on every store the wave has in flight (vmcnt)
        LaneCtx cl = c;
        if constexpr (G::LANE_OPAQUE) {
            int ol = c.lane;
            asm volatile("" : "+v"(ol));
            cl.lane = ol;
            cl.env = c.wave_first + ol;
        }
        const cs_traj_out& out = A.out;
        uint8_t* obs = (uint8_t*)out.obs;
        uint8_t* legal = (uint8_t*)out.legal;
        uint8_t* player = (uint8_t*)out.player;
        float* reward = (float*)out.reward;
        uint8_t* done_o = (uint8_t*)out.done;
        const uint64_t seed = A.seed, t0 = A.t0;

        const int64_t rowbase = (int64_t)t * n;
        const int p = g.current();
        const legal_t<G> lg = g.legal();
        uint32_t bits[G::NB];
        g.observe(p, bits);
        // each row stored where it is produced (round 5: the rows after the step's refill / restage loads ran 6-7 %
        // slower on every torch allocation, profiles/EXPERIMENTS.md)
        const uint32_t pr = pol.at(seed, genv0, t0 + (uint64_t)t, t == 0);
        int a;
        static_assert(G::A <= 256, "the policy pick takes a legal mask of one, two or four 64-bit words");
        if constexpr (G::A > 128) a = pick_legal256(lg, pr);
        else if constexpr (G::A > 64) a = pick_legal128(lg, pr);
        else if constexpr (G::A <= 8) a = pick_legal_small<G::A>((uint32_t)lg, pr);
        else if constexpr (G::A <= 32) a = pick_legal32((uint32_t)lg, pr);
        else a = pick_legal64(lg, pr);
        if constexpr (POL) {
            // the seats' policies are one word of the argument block (a scalar load); the acting seat's byte picks
            // between the random pick above -- always made, at cs_rollout's counter, so random seats play the same
            // games -- and the rule's answer on the state in registers. A rule seat draws nothing.
            const uint32_t pid = (A.seats >> (8 * p)) & 0xFFu;
            int ra;
            if constexpr (G::A <= 32) ra = g.rule_action(pid, p, (uint32_t)lg);
            else ra = g.rule_action(pid, p, lg, pr);   // wide games' rules may pick at random: the step's policy word
            a = pid == (uint32_t)CS_POLICY_RANDOM ? a : ra;
        }
#if !CS_PROF_NO_OBS
        if constexpr (G::SPARSE_K > 0) {
            uint32_t pos[G::SPARSE_K];
            const uint32_t tail = g.observe_pos(p, pos);
            row_write_sparse<G::OBS, G::EPW, G::SPARSE_K, G::RAW_OBS>(
                lds[c.wid], pos, obs + (rowbase + c.wave_first) * G::OBS, cl.lane, c.nvalid, !(flags & 4), tail);
        } else {
            emit_obs<G, G::EPW>(lds[c.wid], bits, obs, rowbase + c.wave_first, flags, cl);
        }
#endif
        // the reward row starts from a zero the compiler cannot hoist out of the loop: a loop-invariant zero pair was
        // kept in a scratch spill whose reload, before each step's reward store, waited on vmcnt(0) -- on gfx950 every
        // store the wave had issued (the obs rows): a drain per step
        uint32_t zr = 0;
        asm volatile("" : "+v"(zr));
        float r[G::P];
#pragma unroll
        for (int k = 0; k < G::P; k++) r[k] = __uint_as_float(zr);
        bool done = false;
        if (c.valid) {
            const int64_t row = rowbase + cl.env;
#if !CS_PROF_NO_SMALL
            emit_legal<G>(legal, row, lg);
            out_store(player + row, (uint8_t)p);
#endif
            if constexpr (G::ACTION_BYTES == 1) out_store((uint8_t*)out.action + row, (uint8_t)a);
            else out_store((int16_t*)out.action + row, (int16_t)a);
            g.step(a, m);
            done = g.is_over();
            if (done) {
                game_payoffs(g, r, m);
                if (out.final_obs) {   // Env.run's final state of every player (envs/env.py:161-164)
#pragma unroll
                    for (int q = 0; q < G::P; q++) {
                        uint32_t fb[G::NB];
                        g.observe(q, fb);
                        write_obs_direct<G>((uint8_t*)out.final_obs + (row * G::P + q) * G::OBS, fb);
                    }
                }
            }
#if !CS_PROF_NO_SMALL
            emit_reward<G>(reward, row, r);
            out_store(done_o + row, (uint8_t)done);
#endif
            if constexpr (DQ == 0) {
                if (done) g.reset(m);
            }
        }
        if constexpr (DQ > 0) {
            // a lane ending its game with an empty queue makes every lane with room draw one deal ahead, in lockstep
            constexpr uint32_t CM = (1u << DqOf<G>::cb) - 1u;   // the header's count field
            if (__ballot(c.valid && done && (q.get(0) & CM) == 0u)) {
                if (c.valid && (q.get(0) & CM) < (uint32_t)DQ) dq_push(g, m, q);
            }
            if (c.valid && done) dq_reset(g, m, q);
        }
        refill(m, cl.lane, flags & 1);
        if (staged) restage<G>(m, stage[c.wid], cl.lane, c.valid);
    }
    bool keep = false;
    if (staged) {
        stage_rows_copy<G::STAGE_W, G::STAGE_PAD>(stage[c.wid], rows, c.lane, c.nvalid, false);
        keep = true;
    }
    if (c.valid) {
        g.store(st, n, c.env);
        if constexpr (DQ > 0) {
#pragma unroll
            for (int w = 0; w < DQW; w++) st[(int64_t)(G::GW + w) * n + c.env] = q.get(w);
        }
        ctl[c.env] = m.ctl_word() | ((uint32_t)keep << 17);
        if (keep) sctl[c.env] = m.sp | (m.sn << 16);
    }
}

// cs_policy_actions: what `policy` plays for the current player of each env, -1 where the game is over; no state or
// stream is written. The random pick is the rollout's at step counter t (philox_u32 = PolicyRng::at).
template <class G>
__global__ __launch_bounds__(BLOCK) void k_policy_actions(const uint32_t* st, int64_t n, int policy, uint64_t seed,
                                                           uint64_t t, uint64_t env_base, int32_t* actions,
                                                           GameParams prm)
{
    const int64_t env = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t* lane_scratch = nullptr;
    if constexpr (G::SCRATCH_WORDS > 0) {   // games whose state lives in LDS (one env per thread, like lane_ctx)
        __shared__ uint32_t scr[WAVES_PER_BLOCK][Scratch<G>::WORDS];
        lane_scratch = scratch_of<G>(scr[threadIdx.x / WAVE], threadIdx.x & (WAVE - 1));
    }
    if (env >= n) return;
    G g;
    g.bind(lane_scratch, prm);
    g.blank();
    g.load(st, n, env);
    int a = -1;
    if (!g.is_over()) {
        if constexpr (G::A > 128) {   // (no game this wide has a rule policy: the ABI refuses any id but CS_POLICY_RANDOM)
            static_assert(G::MAX_POLICY == 0, "rule policies take masks of at most two words");
            a = pick_legal256(g.legal(), philox_u32(seed, env_base + (uint64_t)env, t));
        } else if constexpr (G::A > 64) {
            const Legal128 lg = g.legal();
            const uint32_t pr = philox_u32(seed, env_base + (uint64_t)env, t);
            if constexpr (G::MAX_POLICY > 0) {
                if (policy == CS_POLICY_RANDOM) a = pick_legal128(lg, pr);
                else a = g.rule_action((uint32_t)policy, g.current(), lg, pr);
            } else {
                a = pick_legal128(lg, pr);   // (no rule policy: the ABI refuses any id but CS_POLICY_RANDOM)
            }
        } else if constexpr (G::A <= 32) {
            const uint32_t lg = (uint32_t)g.legal();
            if (policy == CS_POLICY_RANDOM) a = pick_legal_small<G::A>(lg, philox_u32(seed, env_base + (uint64_t)env, t));
            else a = g.rule_action((uint32_t)policy, g.current(), lg);
        } else {
            const uint64_t lg = g.legal();
            const uint32_t pr = philox_u32(seed, env_base + (uint64_t)env, t);
            if constexpr (G::MAX_POLICY > 0) {
                if (policy == CS_POLICY_RANDOM) a = pick_legal64(lg, pr);
                else a = g.rule_action((uint32_t)policy, g.current(), lg, pr);
            } else {
                a = pick_legal64(lg, pr);   // (no rule policy: the ABI refuses any id but CS_POLICY_RANDOM)
            }
        }
    }
    actions[env] = a;
}

// ------------------------------------------------------------------------------------------------------------------
static inline GameParams params_of(const Buffers& b)
{
    return GameParams{b.num_players, b.num_decks, b.chips_for_each, b.dealer_id, b.rng_mode};
}
static inline dim3 grid_for(int64_t n, int epw = WAVE)
{
    const int64_t per = (int64_t)WAVES_PER_BLOCK * epw;
    return dim3((unsigned)((n + per - 1) / per));
}

template <class G>
static hipError_t seed_g(const Buffers& b, const uint32_t* keys, const int32_t* klen, int64_t first, int64_t count,
                         hipStream_t s)
{
    hipLaunchKernelGGL(k_seed<G>, grid_for(count), dim3(BLOCK), 0, s, b.mt, b.ctl, b.state, b.n, keys, klen, first,
                       count, b.kernel_flags, params_of(b));
    return hipGetLastError();
}
template <class G>
static hipError_t reset_g(const Buffers& b, const cs_step_out& o, hipStream_t s)
{
    hipLaunchKernelGGL(k_reset<G>, grid_for(b.n), dim3(BLOCK), 0, s, b.mt, b.ctl, b.state, b.n, o, b.kernel_flags,
                       params_of(b), b.rec);
    return hipGetLastError();
}
template <class G>
static hipError_t step_g(const Buffers& b, const int32_t* a, const cs_step_out& o, hipStream_t s)
{
    hipLaunchKernelGGL(k_step<G>, grid_for(b.n), dim3(BLOCK), 0, s, b.mt, b.ctl, b.state, b.n, a, o, b.kernel_flags,
                       params_of(b), b.rec);
    return hipGetLastError();
}
template <class G>
static hipError_t observe_g(const Buffers& b, int32_t p, const cs_step_out& o, hipStream_t s)
{
    hipLaunchKernelGGL(k_observe<G>, grid_for(b.n), dim3(BLOCK), 0, s, b.state, b.n, p, o, params_of(b), b.rec);
    return hipGetLastError();
}
template <class G>
static hipError_t rollout_g(const Buffers& b, int32_t T, uint64_t seed, uint64_t t0, uint64_t env_base,
                            const cs_traj_out& o, hipStream_t s)
{
    const RolloutArgs a{b.mt, b.ctl, b.state, b.n, seed, t0, env_base, o, params_of(b), b.sctl, b.sbuf, T, b.kernel_flags};
    hipLaunchKernelGGL(k_rollout<G>, grid_for(b.n, G::EPW), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

template <class G>
static hipError_t rollout_policy_g(const Buffers& b, int32_t T, uint64_t seed, uint64_t t0, uint64_t env_base,
                                   uint32_t seats, const cs_traj_out& o, hipStream_t s)
{
    const RolloutArgs a{b.mt, b.ctl, b.state, b.n, seed, t0, env_base, o, params_of(b), b.sctl, b.sbuf, T, b.kernel_flags,
                        seats, 0u};
    hipLaunchKernelGGL((k_rollout<G, true>), grid_for(b.n, G::EPW), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}
template <class G>
static hipError_t policy_actions_g(const Buffers& b, int32_t policy, uint64_t seed, uint64_t t, uint64_t env_base,
                                   int32_t* actions, hipStream_t s)
{
    hipLaunchKernelGGL(k_policy_actions<G>, dim3((unsigned)((b.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, b.state,
                       b.n, policy, seed, t, env_base, actions, params_of(b));
    return hipGetLastError();
}

template <class G>
static void fill_info(cs_game_info* info)
{
    info->obs_dim = G::OBS;
    info->num_actions = G::A;
    info->num_players = G::P;
    info->legal_bytes = G::LB;
    info->action_bytes = G::ACTION_BYTES;
    info->state_words = G::WORDS;
    info->action_feature_dim = G::A;
    info->rng_period = (int32_t)RING;
    info->deal_queue_depth = DqOf<G>::value;
    info->game_words = G::WORDS - DqOf<G>::words;
    info->envs_per_wave = G::EPW;
}

// The launch table entry (cs_engine.h) of skeleton game G. Naming it instantiates the five kernels for G (and the two
// policy kernels of a game with rule policies).
template <class G>
static const GameOps* ops_of()
{
    static const GameOps ops = [] {
        GameOps o{seed_g<G>, reset_g<G>, step_g<G>, observe_g<G>, rollout_g<G>, {}, G::STAGE_W,
                  RING_ENV_WORDS, false, false};
        fill_info<G>(&o.info);
        if constexpr (G::MAX_POLICY > 0) {   // naming them instantiates the two policy kernels for G
            o.rollout_policy = rollout_policy_g<G>;
            o.policy_actions = policy_actions_g<G>;
            o.max_policy = G::MAX_POLICY;
        } else if constexpr (G::RANDOM_ACTIONS) {
            o.policy_actions = policy_actions_g<G>;   // CS_POLICY_RANDOM only (max_policy stays 0)
        }
        return o;
    }();
    return &ops;
}

}  // namespace cs
