// cs_prof.h -- PROFILING BUILDS ONLY. Each macro below, set on an A/B build (`make variant NAME=x
// DEFS=-DCS_PROF_NO_OBS=1`), drops one piece of a kernel so that its share of the launch time can be measured. Such a
// build's outputs are WRONG: it is never the product library (libcardsim.so is built with every macro at 0), and
// bench.py marks a line measured on any other library as a non-product build. The measured splits are in DESIGN.md and
// profiles/EXPERIMENTS.md.
#pragma once

#ifndef CS_PROF_NO_OBS
#define CS_PROF_NO_OBS 0       // k_rollout (cs_skeleton.h): no obs rows
#endif
#ifndef CS_PROF_NO_SMALL
#define CS_PROF_NO_SMALL 0     // k_rollout: no legal / player / reward / done rows
#endif
#ifndef CS_PROF_NO_RESET
#define CS_PROF_NO_RESET 0     // Leduc: no deal at a reset (wrong deals)
#endif
#ifndef CS_PROF_NO_EVAL
#define CS_PROF_NO_EVAL 0      // Limit / No-limit: no showdown evaluator
#endif
#ifndef CS_PROF_NO_DEAL9
#define CS_PROF_NO_DEAL9 0     // Limit / No-limit: no tracked draws of the nine dealt positions
#endif
#ifndef CS_PROF_NO_TRACK
#define CS_PROF_NO_TRACK 0     // Limit / No-limit: no swap trace-back of the dealt cards
#endif
#ifndef CS_PROF_NO_SKIP
#define CS_PROF_NO_SKIP 0      // Limit / No-limit: no skip scan of the 42 undealt draws
#endif
#ifndef CS_PROF_MIXED_WRITER
// Bridge's obs rows (cs_skeleton.h write_obs_mixed; right outputs): 0 the product's aligned pieces, 1 a byte loop the
// compiler merges into unaligned wide stores (profiles/EXPERIMENTS.md B-1 has the other two writers measured)
#define CS_PROF_MIXED_WRITER 0
#endif
#ifndef CS_PROF_MIXED_NT
#define CS_PROF_MIXED_NT 0     // Bridge's obs rows with nontemporal stores (write_obs_mixed_head; right outputs)
#endif
#ifndef CS_PROF_BRIDGE_WAVES
#define CS_PROF_BRIDGE_WAVES 0 // > 0: Bridge k_rollout's waves per SIMD instead of Bridge::MIN_WAVES (right outputs)
#endif
#ifndef CS_PROF_MIXED16_NT
#define CS_PROF_MIXED16_NT 0   // Scout's obs rows (write_obs_mixed16) with nontemporal stores (right outputs)
#endif
#ifndef CS_PROF_SCOUT_MASK
// Scout's legal mask (cs_scout.h; right outputs): 0 the product (built once per step from the 15 neighbour comparisons,
// kept in the lane's LDS scratch), 1 rebuilt by every legal() call, 2 once per step but slice by slice
#define CS_PROF_SCOUT_MASK 0
#endif
#ifndef CS_PROF_SCOUT_WAVES
#define CS_PROF_SCOUT_WAVES 0  // > 0: Scout k_rollout's waves per SIMD instead of Scout::MIN_WAVES (right outputs)
#endif
#ifndef CS_PROF_DDZ
#define CS_PROF_DDZ 0          // DouDizhu k_rollout2: bit 0 no legal rows, bit 1 no obs rows
#endif
