// cs_dqn.h -- internal interface between the C ABI (cs_abi.cpp) and the DQN kernels (cs_dqn.hip): the fused Q-network
// policy kernel, the device replay ring and the Double-DQN target kernel.
#pragma once
#include "cs_engine.h"

namespace cs {

// Replay ring of a handle (cs_replay): `cap` transition slots and one pending row per (env, seat), all in one allocation
struct ReplayRing {
    int64_t cap;
    int32_t O, LB, P, abytes;   // obs bytes, legal-mask bytes, players, bytes per trajectory action
    uint8_t* st;                // [cap][O] state
    uint8_t* nst;               // [cap][O] next_state
    uint8_t* nlg;               // [cap][LB] next state's legal mask (0 on a terminal transition)
    int32_t* act;               // [cap]
    float* rew;                 // [cap]
    uint8_t* dne;               // [cap]
    int64_t* total;             // [1] transitions ever appended (slot of transition i: i % cap)
    uint8_t* pvalid;            // [n * P] 1: (env, seat) holds a pending row
    uint8_t* pst;               // [n * P][O] the pending row's state
    int32_t* pact;              // [n * P] its action
    int32_t* newpend;           // [n * P] row t of the push's window that becomes the seat's pending row, -1 none
};

// dynamic LDS bytes of a k_qnet block for this net (both activation buffers of its 64 rows and the weight tile)
int64_t qnet_lds_bytes(const cs_qnet& net);
hipError_t launch_qnet(const cs_qnet& net, const uint8_t* obs, const uint8_t* legal, const uint8_t* done, int64_t rows,
                       float eps, uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions, float* q,
                       hipStream_t s);
// code: [n * P + T * n + 1] i32, pos: the same length (scratch of the push, grown by the caller)
hipError_t launch_replay_push(const Buffers& b, const ReplayRing& r, int32_t T, const cs_traj_out& tr,
                              uint32_t seat_mask, int32_t* code, int32_t* pos, void** tmp, size_t* tmp_bytes,
                              hipStream_t s);
hipError_t launch_replay_gather(const ReplayRing& r, const int64_t* idx, int64_t B, const cs_replay_batch& o,
                                hipStream_t s);
hipError_t launch_dqn_targets(const float* q_next, const float* q_next_target, const uint8_t* next_legal,
                              const float* reward, const uint8_t* done, int64_t B, int32_t A, float gamma,
                              float* target, int32_t* best, hipStream_t s);

}  // namespace cs
