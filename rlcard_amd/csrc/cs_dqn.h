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
// the descriptor read as Linear/ReLU with the average-policy head (softmax, remove_illegal, a sampled action)
hipError_t launch_pnet(const cs_qnet& net, const uint8_t* obs, const uint8_t* legal, const uint8_t* done, int64_t rows,
                       uint64_t seed, uint64_t t, uint64_t row_base, int32_t* actions, float* probs, hipStream_t s);
// mode u8 [rows]: 1 the Q-network's epsilon-greedy action, 0 the average policy's sampled one; the rows are compacted
// into one list per network in `scratch` (nfsp_scratch_bytes(rows) bytes, 256-B aligned) and each network runs over
// its list
hipError_t nfsp_scratch_bytes(int64_t rows, size_t* bytes);
hipError_t launch_nfsp_actions(const cs_qnet& qnet, const cs_qnet& pnet, const uint8_t* obs, const uint8_t* legal,
                               const uint8_t* done, const uint8_t* mode, int64_t rows, float eps, uint64_t seed,
                               uint64_t t, uint64_t row_base, int32_t* actions, float* probs, void* scratch,
                               hipStream_t s);

// Reservoir buffer of a handle (cs_reservoir, cs_nfsp.hip): `cap` slots of (state, action id)
struct Reservoir {
    int64_t cap;
    int32_t O, P, A, abytes;    // obs bytes, players, actions, bytes per trajectory action
    uint64_t seed;              // key of the replacement draws
    uint8_t* st;                // [cap][O] state
    int32_t* act;               // [cap] action id (the one-hot action_probs row)
    unsigned long long* occ;    // [cap] stream index + 1 of the slot's occupant, 0 = empty
    int64_t* add_calls;         // [1] candidates ever offered (ReservoirBuffer._add_calls)
};
// pos: [T * n + 1] i32 scratch of the push (grown by the caller)
hipError_t launch_reservoir_push(const Reservoir& r, int32_t T, int64_t n, const uint8_t* obs, const uint8_t* player,
                                 const void* action, const uint8_t* mode, uint32_t seat_mask, int32_t* pos, DevBuf& scan,
                                 hipStream_t s);
hipError_t launch_reservoir_gather(const Reservoir& r, const int64_t* idx, int64_t B, float* state, float* probs,
                                   hipStream_t s);

// code: [n * P + T * n + 1] i32, pos: the same length (scratch of the push, grown by the caller)
hipError_t launch_replay_push(const Buffers& b, const ReplayRing& r, int32_t T, const cs_traj_out& tr,
                              uint32_t seat_mask, int32_t* code, int32_t* pos, DevBuf& scan, hipStream_t s);
hipError_t launch_replay_gather(const ReplayRing& r, const int64_t* idx, int64_t B, const cs_replay_batch& o,
                                hipStream_t s);
hipError_t launch_dqn_targets(const float* q_next, const float* q_next_target, const uint8_t* next_legal,
                              const float* reward, const uint8_t* done, int64_t B, int32_t A, float gamma,
                              float* target, int32_t* best, hipStream_t s);

// cs_dqn_train.hip: dynamic LDS bytes of the one k_dqn_train workgroup for this net at batch size B
int64_t dqn_train_lds_bytes(const cs_dqn_net& net, int32_t B);
hipError_t launch_dqn_train(const ReplayRing& r, const cs_dqn_net& qnet, const cs_dqn_net& target,
                            const cs_dqn_adam& opt, const cs_dqn_train_args& args, hipStream_t s);

}  // namespace cs
