// cs_device.h -- device building blocks shared by every game kernel (gfx950 / CDNA4, wave64).
//
// Per-env RNG contract: numpy's legacy RandomState (MT19937) seeded by init_by_array with the key of
// rlcard/utils/seeding.py:33-113, never re-seeded across resets (rlcard/envs/env.py:228-231). This header holds the
// MT19937 arithmetic every layout shares (init_by_array, the in-place twist, mix, temper). How an env's stream is kept
// in HBM is the game's: the lane-per-env games' ring of tempered low bytes (cs_ring.h), DouDizhu's two word blocks
// (cs_doudizhu.hip, WaveMt), the Blackjack shoe's word column (cs_blackjack_shoe.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "cs_prof.h"

namespace cs {

// rollout output stores: nontemporal (streamed past the caches: written once, GBs per launch, read by the consumer
// long after), measured faster than default-policy stores (Leduc 2.37 -> 2.08 ms, Limit 1.39 -> 1.33 ms per launch)
// and than explicit gfx950 cache-policy bits (round 5, profiles/EXPERIMENTS.md)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void out_store16(uint4* p, const uint4& v)
{
    const u32x4_t x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, (u32x4_t*)p);
}
template <class T>
__device__ __forceinline__ void out_store(T* p, T v)
{
    __builtin_nontemporal_store(v, p);
}

constexpr int MT_N = 624;
constexpr int MT_M = 397;
constexpr int WAVE = 64;

// runtime game configuration (cs_config): blackjack reads players / decks, no-limit hold'em stacks / dealer
struct GameParams {
    int32_t num_players;
    int32_t num_decks;
    int32_t chips_for_each;   // no-limit: stack per player
    int32_t dealer_id;        // no-limit: -1 = drawn by the first reset (rlcard's None), else fixed
    int32_t rng_mode;         // CS_RNG_MT19937 (reference-compatible) or CS_RNG_PHILOX (cs_ring.h)
};

// What a skeleton game type (cs_skeleton.h) inherits unless it states otherwise
struct GameDefaults {
    // k_rollout: the lane id made opaque at every step. Round 5, same box: Limit 8.18 -> 8.07 ms and No-limit 9.33 ->
    // 9.10 without it, Blackjack 20.62 -> 20.89 and Leduc even
    static constexpr bool LANE_OPAQUE = true;
    // the 8-B reward row's value made opaque before its nontemporal store: without it the optimizer may split the store
    // back into two float stores and drop the nontemporal hint on the way (No-limit's rollout); with it where the hint
    // survives anyway (Leduc, Limit) the step schedules worse (Leduc 4.23 -> 4.48 ms, round 5)
    static constexpr bool REWARD_OPAQUE = false;
    // Env.get_payoffs at the step that ends the game takes the lane's RNG: games whose judge may draw from the env's
    // stream (N-player hold'em's odd split remainders, limitholdem/judger.py:80-83)
    static constexpr bool PAYOFF_DRAWS = false;
    static constexpr int SPARSE_K = 0;     // > 0: obs rows are one-hot with SPARSE_K known positions (observe_pos)
    static constexpr int MAX_POLICY = 0;   // > 0: the largest CS_POLICY_* id of the game's rule_action
    // cs_policy_actions' random pick for a game without rule policies (MAX_POLICY 0 otherwise has no policy kernels)
    static constexpr bool RANDOM_ACTIONS = false;
    static constexpr int DQ = 0;           // > 0: deals drawn ahead into a queue of this depth (cs_dq.h)
    // obs rows stored by their own lane, 16 B at a time, instead of through the wave's LDS span image: for games whose
    // occupancy is bound by LDS and whose rows are dword multiples (UNO: the 60 KB image per block was one block per CU;
    // a row that is no 16-B multiple, Gin Rummy's 260 B, finds its own 16-B boundary)
    static constexpr bool OBS_DIRECT = false;
    // > 0: a direct 0/1 row that holds RAW_SPAN_LEN raw bytes from byte RAW_SPAN_AT on (Bridge's bidding_rep of action
    // ids): observe() gives the bitmap in G::NBITS words, zero over the span, then the span's bytes four per word, and
    // the row may have any length (cs_skeleton.h write_obs_mixed)
    static constexpr int RAW_SPAN_LEN = 0, RAW_SPAN_AT = 0;
};

__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

// the low byte of mt_temper(y) (bits 8.. differ): the last two steps only reach the low byte through bits 0..10 and
// 18..25 of the second step's value y2, as y2 ^ (y2 >> 18) ^ ((y2 >> 3) & 0xF1) -- no left shift (a quarter-rate
// instruction on gfx950) in the third step. Both maps are GF(2)-linear; equal on the 32 unit vectors.
__device__ __forceinline__ uint32_t mt_temper_lo8(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    return y ^ (y >> 18) ^ ((y >> 3) & 0xF1u);
}

__device__ __forceinline__ uint32_t mt_mix(uint32_t cur, uint32_t nxt, uint32_t far)
{
    // (cur & 0x80000000) | (nxt & 0x7fffffff) as one bitfield insert (v_bfi_b32) instead of and + and_or; y & 1 is
    // nxt & 1, so the matrix term does not wait for the insert
    uint32_t y;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(y) : "s"(0x7fffffffu), "v"(nxt), "v"(cur));
    return far ^ (y >> 1) ^ ((0u - (nxt & 1u)) & 0x9908b0dfu);
}

// The 624 state words behind `mt`: a plain pointer, or an accessor with get(k) / set(k, v) (the shoe's Col)
template <class M>
__device__ __forceinline__ uint32_t mt_get(M mt, int k)
{
    if constexpr (std::is_pointer<M>::value) return mt[k];
    else return mt.get(k);
}
template <class M>
__device__ __forceinline__ void mt_set(M mt, int k, uint32_t v)
{
    if constexpr (std::is_pointer<M>::value) mt[k] = v;
    else mt.set(k, v);
}

// numpy init_by_array (mt19937_init_by_array); the state then awaits its first twist
template <class M>
__device__ inline void mt_init_by_array(M mt, const uint32_t* key, int klen)
{
    uint32_t prev = 19650218u;
    mt_set(mt, 0, prev);
    for (int i = 1; i < MT_N; i++) {
        prev = 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i;
        mt_set(mt, i, prev);
    }
    int i = 1, j = 0;
    prev = mt_get(mt, 0);
    for (int k = MT_N; k; k--) {
        const uint32_t v = (mt_get(mt, i) ^ ((prev ^ (prev >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        mt_set(mt, i, v);
        prev = v;
        i++;
        j++;
        if (i >= MT_N) { mt_set(mt, 0, mt_get(mt, MT_N - 1)); prev = mt_get(mt, 0); i = 1; }
        if (j >= klen) j = 0;
    }
    for (int k = MT_N - 1; k; k--) {
        const uint32_t v = (mt_get(mt, i) ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
        mt_set(mt, i, v);
        prev = v;
        i++;
        if (i >= MT_N) { mt_set(mt, 0, mt_get(mt, MT_N - 1)); prev = mt_get(mt, 0); i = 1; }
    }
    mt_set(mt, 0, 0x80000000u);
}

// numpy's twist (genrand_int32's reload), in place: mt[k] only reads mt[k+1], mt[k+397] (not yet rewritten) and the
// already-new mt[k-227]
template <class M>
__device__ inline void mt_twist_inplace(M mt)
{
    for (int k = 0; k < MT_N - MT_M; k++) mt_set(mt, k, mt_mix(mt_get(mt, k), mt_get(mt, k + 1), mt_get(mt, k + MT_M)));
    for (int k = MT_N - MT_M; k < MT_N - 1; k++)
        mt_set(mt, k, mt_mix(mt_get(mt, k), mt_get(mt, k + 1), mt_get(mt, k + MT_M - MT_N)));
    mt_set(mt, MT_N - 1, mt_mix(mt_get(mt, MT_N - 1), mt_get(mt, 0), mt_get(mt, MT_M - 1)));
}

// Global-address-space view of a pointer into HBM: pointers rebuilt from integers (readlane) are generic, and generic
// accesses compile to flat_load/flat_store, which count on lgkmcnt too, so every use waits with vmcnt(0) lgkmcnt(0)
// -- draining the wave's outstanding trajectory stores each time (measured in the k_rollout ISA)
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(1))) uint8_t gu8;

// 64-bit pointer held by lane j (readlane returns int: go through uint32_t so bit 31 of the low half is not
// sign-extended into the high half)
__device__ __forceinline__ gu32* lane_ptr(uint32_t* p, int j)
{
    const uint64_t b = (uint64_t)(uintptr_t)p;
    const uint64_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, j);
    const uint64_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), j);
    return (gu32*)(uintptr_t)(lo | (hi << 32));
}

// How a lane's view of its env's byte ring (cs_ring.h RingLane<MODE>) serves draws:
//   STAGE_NONE  one global load per draw (single-step kernels: staging would cost more than it saves);
//   STAGE_LDS   W staged bytes in a per-lane LDS row (the rollout kernels).
// Why staging: lanes sit at different stream positions, so one load per draw is a 64-line gather per wave
// instruction, and a reset's rejection loops issue one such gather per trip of the slowest lane (rocprofv3 on
// k_rollout<Leduc>: TA busy 68% of the kernel, ~300 L1 accesses per wave-step, waves waiting 80% of their cycles).
// Every draw of the lane-per-env games is random_interval(max <= 53), which looks only at the low 8 bits of the
// tempered word, so at step boundaries (after the refill) lanes running low restage their next ring bytes; draws then
// read LDS, global only as a fallback when a lane outruns its stage.
// Measured on MI355X (tools/ab_rollout.py): staging beat one load per draw by 13-30 %; register variants (a per-draw
// 8-word window, 8/16-word bursts inside the reset, 16 staged bytes in 4 VGPRs) all lost to it.
enum { STAGE_NONE = 0, STAGE_LDS = 2 };

// STAGE_LDS rows: W bytes per lane (W multiple of 64), row stride W + PAD (per game): LDS bounds occupancy, so the
// pad is as small as the measurements allow (steady-state A/B on MI355X: Leduc W 64 + 4 fits 6 blocks per CU and is
// 13 % faster than W + 16; Limit W 128 + 8 fits 3 blocks per CU where + 16 fitted 2, and beats + 4 by 1.5 %). The
// persist copies move 16 / 8 / 4 B per lane, whatever the stride allows.
template <int W, int PAD, int ROWS = WAVE>
struct Stage {
    static_assert(W % 16 == 0 && WAVE % (W / 4) == 0, "a staged row is copied by W / 4 lanes of one wave instruction");
    static_assert(PAD % 4 == 0, "rows are written as dwords");
    static constexpr int STRIDE = W + PAD;
    static constexpr int CHUNK = STRIDE % 16 == 0 ? 16 : (STRIDE % 8 == 0 ? 8 : 4);   // bytes per persist copy
    static constexpr int BYTES = ROWS * STRIDE + 16;   // + 16: Leduc's reset reads a 20-B window at any row offset
};

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Persist / restore a wave's staging rows (W bytes per env, HBM row-major [env][W]) with coalesced 16-B / 8-B copies, so a
// launch does not restage every lane from scratch. nvalid = envs of this wave.
template <int W, int PAD>
__device__ __forceinline__ void stage_rows_copy(uint8_t* area, uint8_t* hbm_rows, int lane, int nvalid, bool to_lds)
{
    constexpr int STRIDE = Stage<W, PAD>::STRIDE, CH = Stage<W, PAD>::CHUNK, CPR = W / CH;   // chunks per row
#pragma unroll
    for (int i = 0; i < CPR; i++) {
        const int q = i * WAVE + lane, row = q / CPR, col = q - row * CPR;
        if (row < nvalid) {
            uint8_t* l = area + row * STRIDE + col * CH;
            uint8_t* g = hbm_rows + (size_t)q * CH;
            if constexpr (CH == 16) {
                if (to_lds) *(uint4*)l = *(const uint4*)g;
                else *(uint4*)g = *(const uint4*)l;
            } else if constexpr (CH == 8) {
                if (to_lds) *(uint2*)l = *(const uint2*)g;
                else *(uint2*)g = *(const uint2*)l;
            } else {
                if (to_lds) *(uint32_t*)l = *(const uint32_t*)g;
                else *(uint32_t*)g = *(const uint32_t*)l;
            }
        }
    }
    wave_sync_lds();
}

// ---- Philox4x32-10 policy RNG: counter (env, t), key = policy seed. Identical to oracle/or_rng.c. ---------------
__device__ __forceinline__ void philox4(uint64_t seed, uint64_t env, uint64_t blk, uint32_t (&out)[4])
{
    uint32_t c0 = (uint32_t)env, c1 = (uint32_t)(env >> 32), c2 = (uint32_t)blk, c3 = (uint32_t)(blk >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// The policy's u32 for (env, step t): word t % 4 of Philox4x32-10(key = seed, counter = (env, t / 4)), so one block
// serves four consecutive steps (PolicyRng keeps it in registers across steps). Identical to oracle/or_rng.c.
__device__ __forceinline__ uint32_t philox_u32(uint64_t seed, uint64_t env, uint64_t t)
{
    uint32_t w[4];
    philox4(seed, env, t >> 2, w);
    const uint32_t q = (uint32_t)t & 3u;
    return q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
}

struct PolicyRng {
    uint32_t w0, w1, w2, w3;
    // the u32 of absolute step t; steps are visited in order, a new block every fourth one
    __device__ __forceinline__ uint32_t at(uint64_t seed, uint64_t env, uint64_t t, bool first)
    {
        const uint32_t q = (uint32_t)t & 3u;
        if (first || q == 0) {
            uint32_t w[4];
            philox4(seed, env, t >> 2, w);
            w0 = w[0]; w1 = w[1]; w2 = w[2]; w3 = w[3];
        }
        return q == 0 ? w0 : (q == 1 ? w1 : (q == 2 ? w2 : w3));
    }
};

// uniform pick among the set bits of a <= 32-action legal mask (k = floor(r * count / 2^32), k-th set bit)
__device__ __forceinline__ int pick_legal32(uint32_t legal, uint32_t r)
{
    const int count = __popc(legal);
    if (count == 0) return -1;
    int k = (int)__umulhi(r, (uint32_t)count);
    while (k--) legal &= legal - 1;
    return __builtin_ctz(legal);
}
// the same pick over a <= 64-action legal mask (UNO's 61 ids)
__device__ __forceinline__ int pick_legal64(uint64_t legal, uint32_t r)
{
    const int count = __popcll(legal);
    if (count == 0) return -1;
    int k = (int)__umulhi(r, (uint32_t)count);
    while (k--) legal &= legal - 1;
    return __builtin_ctzll(legal);
}
// A legal mask of 65..128 actions (Gin Rummy's 110 ids): id i is bit i % 64 of lo (i < 64) or hi. Games of at most 64
// actions keep a plain uint64_t (cs_skeleton.h legal_t).
struct Legal128 {
    uint64_t lo, hi;
};
__device__ __forceinline__ bool legal_empty(const Legal128& m) { return (m.lo | m.hi) == 0ull; }
__device__ __forceinline__ bool legal_has(const Legal128& m, int a) { return ((a < 64 ? m.lo : m.hi) >> (a & 63)) & 1ull; }
__device__ __forceinline__ int legal_lowest(const Legal128& m)
{
    return m.lo ? __builtin_ctzll(m.lo) : 64 + __builtin_ctzll(m.hi);
}
// pick_legal64's formula over both words: the k-th set bit in id order, k = floor(r * count / 2^32)
__device__ __forceinline__ int pick_legal128(const Legal128& legal, uint32_t r)
{
    const int clo = __popcll(legal.lo), count = clo + __popcll(legal.hi);
    if (count == 0) return -1;
    int k = (int)__umulhi(r, (uint32_t)count);
    const bool high = k >= clo;
    uint64_t w = high ? legal.hi : legal.lo;
    k -= high ? clo : 0;
    while (k--) w &= w - 1;
    return (high ? 64 : 0) + __builtin_ctzll(w);
}
// A legal mask of 129..256 actions (Scout's 204 ids): id i is bit i % 64 of w[i / 64]. The words are only ever indexed
// by constants, so the mask lives in registers.
struct Legal256 {
    uint64_t w[4];
};
__device__ __forceinline__ bool legal_empty(const Legal256& m) { return (m.w[0] | m.w[1] | m.w[2] | m.w[3]) == 0ull; }
__device__ __forceinline__ uint64_t legal_word(const Legal256& m, int k)
{
    return k == 0 ? m.w[0] : (k == 1 ? m.w[1] : (k == 2 ? m.w[2] : m.w[3]));
}
__device__ __forceinline__ bool legal_has(const Legal256& m, int a) { return (legal_word(m, a >> 6) >> (a & 63)) & 1ull; }
__device__ __forceinline__ int legal_lowest(const Legal256& m)
{
    if (m.w[0]) return __builtin_ctzll(m.w[0]);
    if (m.w[1]) return 64 + __builtin_ctzll(m.w[1]);
    if (m.w[2]) return 128 + __builtin_ctzll(m.w[2]);
    return 192 + __builtin_ctzll(m.w[3]);
}
// pick_legal64's formula over the four words: the k-th set bit in id order, k = floor(r * count / 2^32)
__device__ __forceinline__ int pick_legal256(const Legal256& legal, uint32_t r)
{
    const int c0 = __popcll(legal.w[0]), c1 = c0 + __popcll(legal.w[1]), c2 = c1 + __popcll(legal.w[2]);
    const int count = c2 + __popcll(legal.w[3]);
    if (count == 0) return -1;
    int k = (int)__umulhi(r, (uint32_t)count);
    const int q = k < c0 ? 0 : (k < c1 ? 1 : (k < c2 ? 2 : 3));
    uint64_t w = legal_word(legal, q);
    k -= q == 0 ? 0 : (q == 1 ? c0 : (q == 2 ? c1 : c2));
    while (k--) w &= w - 1;
    return 64 * q + __builtin_ctzll(w);
}
// the same pick for masks of at most A bits (A <= 8), branch-free: the k-th set bit after k clears of the lowest
// (k < A), so a wave's lanes never loop to the largest k among them
template <int A>
__device__ __forceinline__ int pick_legal_small(uint32_t legal, uint32_t r)
{
    static_assert(A >= 1 && A <= 8, "small action sets");
    const uint32_t count = (uint32_t)__popc(legal);
    const uint32_t k = __umulhi(r, count);
#pragma unroll
    for (uint32_t i = 0; i + 1 < (uint32_t)A; i++) legal = i < k ? legal & (legal - 1u) : legal;
    return count == 0 ? -1 : __builtin_ctz(legal);
}

// ---- coalesced output of per-lane byte rows ------------------------------------------------------------------------
// A wave's 64 envs own 64 consecutive rows of `ROW` bytes in every [.., N, ROW] output, i.e. one contiguous
// 64*ROW-byte span. Lanes build their row as bit-planes (bit b of bits[] = byte b is 1), expand it to bytes in
// registers, stage it through LDS (odd dword stride: conflict-free ds_write_b32), and the wave writes the span
// with 256-B dword stores.
template <int ROW, int ROWS = WAVE>   // ROWS: envs (rows) per wave, lanes >= ROWS hold none
struct RowWriter {
    static_assert(ROW % 4 == 0, "byte rows must be dword multiples");
    static constexpr int DW = ROW / 4;
    static constexpr int LDS_WORDS = ROWS * DW;   // the LDS image IS the output span (row-major, no padding)
    static constexpr int NB = (ROW + 31) / 32;
    static constexpr int Q = (ROWS * DW) / 4;     // 16-B pieces in a full span

    // 4 bits -> 4 bytes of 0/1: x * (1 + 2^7 + 2^14 + 2^21) puts bit i at bit 8i and the four shifted copies of a
    // 4-bit x never overlap (bits 0-3, 7-10, 14-17, 21-24), so one 24-bit multiply + mask does it
    __device__ static __forceinline__ uint32_t expand4(uint32_t x)
    {
        return __umul24(x & 15u, 0x204081u) & 0x01010101u;
    }

    // bits: NB words of a one-bit-per-byte bitmap; out_span: first byte of the wave's 64 rows; nvalid rows written.
    // LDS writes use an odd stride when DW is odd (conflict-free) and 2-way at worst otherwise; the span leaves LDS
    // with ds_read_b128 and goes out with 16-B stores (dword stores if the span is not 16-B aligned or partial).
    __device__ static __forceinline__ void write(uint32_t* lds, const uint32_t (&bits)[NB], uint8_t* out_span,
                                                 int lane, int nvalid, bool wide = true)
    {
        if (lane < ROWS) {
#pragma unroll
            for (int j = 0; j < DW; j++) lds[lane * DW + j] = expand4(bits[j / 8] >> (4 * (j % 8)));
        }
        write_out(lds, bits, out_span, lane, nvalid, wide);
    }
    // the span image in LDS (written by this wave) to the output span
    __device__ static __forceinline__ void write_out(uint32_t* lds, const uint32_t (&)[NB], uint8_t* out_span,
                                                     int lane, int nvalid, bool wide)
    {
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (wide && nvalid == ROWS && (((uintptr_t)out_span) & 15u) == 0) {
            uint4* o = (uint4*)out_span;
            const uint4* src = (const uint4*)lds;
#pragma unroll
            for (int j = 0; j < (Q + WAVE - 1) / WAVE; j++) {
                const int q = j * WAVE + lane;
                if (q < Q) out_store16(o + q, src[q]);
            }
        } else {
            uint32_t* o = (uint32_t*)out_span;
            const int total = nvalid * DW;
#pragma unroll
            for (int j = 0; j < DW; j++) {
                const int e = j * WAVE + lane;
                if (e < total) o[e] = lds[e];
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

// Same span writer for rows of raw byte values (ROW even): words[] holds the row's bytes four per word (byte k in
// byte k % 4 of words[k / 4]); lanes write their row into the LDS image as 16-bit pieces (ROW % 4 == 2) or dwords,
// and the span leaves with 16-B stores when it is a whole, aligned number of 16-B pieces.
template <int ROW, int ROWS = WAVE>
struct RowWriterRaw {
    static_assert(ROW % 2 == 0, "raw rows are staged as 16-bit pieces");
    static constexpr int NW = (ROW + 3) / 4;
    static constexpr int SPAN = ROWS * ROW;
    static constexpr int LDS_WORDS = (SPAN + 3) / 4;

    __device__ static __forceinline__ void write(uint32_t* lds, const uint32_t (&words)[NW], uint8_t* out_span,
                                                 int lane, int nvalid, bool wide = true)
    {
        if (lane < ROWS) {
            if constexpr (ROW % 4 == 0) {
#pragma unroll
                for (int j = 0; j < ROW / 4; j++) lds[lane * (ROW / 4) + j] = words[j];
            } else {
                uint16_t* l16 = (uint16_t*)lds + lane * (ROW / 2);
#pragma unroll
                for (int j = 0; j < ROW / 2; j++) l16[j] = (uint16_t)(words[j / 2] >> (16 * (j & 1)));
            }
        }
        write_out(lds, out_span, lane, nvalid, wide);
    }
    __device__ static __forceinline__ void write_out(uint32_t* lds, uint8_t* out_span, int lane, int nvalid, bool wide)
    {
        wave_sync_lds();
        const int bytes = nvalid * ROW;
        if (SPAN % 16 == 0 && wide && nvalid == ROWS && (((uintptr_t)out_span) & 15u) == 0) {
            uint4* o = (uint4*)out_span;
            const uint4* src = (const uint4*)lds;
#pragma unroll
            for (int j = 0; j < (SPAN / 16 + WAVE - 1) / WAVE; j++) {
                const int q = j * WAVE + lane;
                if (q < SPAN / 16) out_store16(o + q, src[q]);
            }
        } else if (bytes % 4 == 0 && (((uintptr_t)out_span) & 3u) == 0) {
            uint32_t* o = (uint32_t*)out_span;
            for (int e = lane; e < bytes / 4; e += WAVE) o[e] = lds[e];
        } else {
            uint16_t* o = (uint16_t*)out_span;
            const uint16_t* src = (const uint16_t*)lds;
            for (int e = lane; e < bytes / 2; e += WAVE) o[e] = src[e];
        }
        wave_sync_lds();
    }
};

// The span writer for one-hot rows with few ones at known positions (Leduc: K = 4 byte positions per row, a repeated
// position for an absent one): the lanes zero the span image with 16-B LDS stores, then write their K ones as byte
// stores (a wave's LDS operations complete in order), instead of expanding every dword of the row (4 VALU + one LDS
// store per dword). The span leaves LDS exactly as write() sends it.
// RAW: the row is raw bytes (RowWriterRaw) whose last two bytes are the 16-bit value `tail` (No-limit's chips); the
// ones sit among the bytes before them.
template <int ROW, int ROWS, int K, bool RAW = false>
__device__ __forceinline__ void row_write_sparse(uint32_t* lds, const uint32_t (&pos)[K], uint8_t* out_span, int lane,
                                                 int nvalid, bool wide, uint32_t tail = 0)
{
    constexpr int SPAN16 = (ROWS * ROW + 15) / 16;
    uint4* z = (uint4*)lds;
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));   // made here: a hoisted zero register ends up in a scratch spill (vmcnt(0) reload)
#pragma unroll
    for (int j = 0; j < (SPAN16 + WAVE - 1) / WAVE; j++) {
        const int q = j * WAVE + lane;
        if (q < SPAN16) z[q] = make_uint4(zero, zero, zero, zero);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < ROWS) {
        uint8_t* row = (uint8_t*)lds + lane * ROW;
#pragma unroll
        for (int k = 0; k < K; k++) row[pos[k]] = 1;
        if constexpr (RAW) *(uint16_t*)(row + ROW - 2) = (uint16_t)tail;   // ROW even: 2-B aligned
    }
    if constexpr (RAW) {
        RowWriterRaw<ROW, ROWS>::write_out(lds, out_span, lane, nvalid, wide);
    } else {
        uint32_t none[RowWriter<ROW, ROWS>::NB];
        RowWriter<ROW, ROWS>::write_out(lds, none, out_span, lane, nvalid, wide);
    }
}

// XCD-aware block order: the dispatcher hands block b to XCD b % 8 (MI355X: 8 XCDs, each with its own L2), so with
// the identity map neighbouring env ranges -- whose trajectory rows share 128-B lines where a row is not a line
// multiple (DouDizhu's 901 / 3 434-byte rows) -- are written through different L2s, and every shared line reaches HBM
// as two partial writes. xcd_block maps block b to env-block x * q + min(x, r) + b / 8 (x = b % 8, nb = 8 q + r): each
// XCD takes one contiguous eighth of the env range. A bijection of [0, nb) for any nb (results do not depend on it).
constexpr int NUM_XCD = 8;
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb)
{
    const uint32_t x = b % NUM_XCD, q = nb / NUM_XCD, r = nb % NUM_XCD;
    return x * q + (x < r ? x : r) + b / NUM_XCD;
}

// set bit p of a multi-word bitmap without dynamic register indexing
template <int NB>
__device__ __forceinline__ void set_bit(uint32_t (&bits)[NB], int p)
{
#pragma unroll
    for (int j = 0; j < NB; j++) bits[j] |= ((p >> 5) == j) ? (1u << (p & 31)) : 0u;
}

// ---- the agents' buffer kernels (cs_dmc.hip, cs_dqn.hip, cs_nfsp.hip) ----------------------------------------------
// row `row` of a trajectory's action tensor: u8 or i16, by cs_game_info.action_bytes
__device__ __forceinline__ int traj_action(const void* action, int abytes, int64_t row)
{
    return abytes == 1 ? (int)((const uint8_t*)action)[row] : (int)((const int16_t*)action)[row];
}

// thread i of a grid with one thread per (row, 4 bytes of the row's O): its row and first byte column; false past the
// last row
__device__ __forceinline__ bool row_col4(int64_t i, int64_t rows, int O, int64_t& row, int& col)
{
    const int q4 = (O + 3) / 4;
    if (i >= rows * q4) return false;
    row = i / q4;
    col = (int)(i - row * q4) * 4;
    return true;
}

// a caller's gather index brought into [0, size) (0 when the buffer is empty), so the kernel reads inside the buffer
__device__ __forceinline__ int64_t clamp_index(int64_t x, int64_t size)
{
    return x < 0 ? 0 : (x >= size ? (size > 0 ? size - 1 : 0) : x);
}

}  // namespace cs
