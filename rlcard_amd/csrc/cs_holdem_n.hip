// cs_holdem_n.hip -- the lockstep skeleton (cs_skeleton.h) instantiated for 3..22-player hold'em (cs_holdem_n.h):
// Leduc 3..5, Limit and No-limit 3..6 here; 7..10, 11..16 and 17..22 in cs_holdem_n10.hip / n16.hip / n22.hip (their
// own translation units: they compile in parallel). find_game (cs_kernels.hip) asks find_holdem_n when
// cs_config.num_players > 2; each unit knows its own player counts and answers null for the others.
#include "cs_skeleton.h"
#include "cs_holdem_n.h"

namespace cs {

const GameOps* find_holdem_n(int32_t game, int32_t np)
{
    for (auto find : {find_holdem_n10, find_holdem_n16, find_holdem_n22})
        if (const GameOps* ops = find(game, np)) return ops;
    switch (game) {
    case CS_GAME_LEDUC:
        switch (np) {
        case 3: return ops_of<LeducN<3>>();
        case 4: return ops_of<LeducN<4>>();
        case 5: return ops_of<LeducN<5>>();
        default: return nullptr;
        }
    case CS_GAME_LIMIT:
        switch (np) {
        case 3: return ops_of<LimitN<3>>();
        case 4: return ops_of<LimitN<4>>();
        case 5: return ops_of<LimitN<5>>();
        case 6: return ops_of<LimitN<6>>();
        default: return nullptr;
        }
    case CS_GAME_NOLIMIT:
        switch (np) {
        case 3: return ops_of<NolimitN<3>>();
        case 4: return ops_of<NolimitN<4>>();
        case 5: return ops_of<NolimitN<5>>();
        case 6: return ops_of<NolimitN<6>>();
        default: return nullptr;
        }
    default: return nullptr;
    }
}

}  // namespace cs
