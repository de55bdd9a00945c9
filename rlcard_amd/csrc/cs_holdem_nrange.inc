// cs_holdem_nrange.inc -- one translation unit's worth of the lockstep skeleton (cs_skeleton.h) instantiated for
// Limit / No-limit hold'em with CS_NP_LO..CS_NP_HI players (cs_holdem_n.h), behind the unit's one export: the finder
// CS_NP_NAME, which cs_holdem_n.hip's find_holdem_n asks for more than 6 players. Included by cs_holdem_n10.hip
// (7..10), cs_holdem_n16.hip (11..16) and cs_holdem_n22.hip (17..22): the big player counts are split over three
// units so that they compile in parallel.
#include "cs_skeleton.h"
#include "cs_holdem_n.h"

namespace cs {

// LimitN<np> / NolimitN<np> for np in [P, HI]; null otherwise
template <int P, int HI>
static const GameOps* np_range(int32_t game, int32_t np)
{
    if constexpr (P > HI) {
        return nullptr;
    } else {
        if (np != P) return np_range<P + 1, HI>(game, np);
        if (game == CS_GAME_LIMIT) return ops_of<LimitN<P>>();
        if (game == CS_GAME_NOLIMIT) return ops_of<NolimitN<P>>();
        return nullptr;
    }
}

const GameOps* CS_NP_NAME(int32_t game, int32_t np) { return np_range<CS_NP_LO, CS_NP_HI>(game, np); }

}  // namespace cs
