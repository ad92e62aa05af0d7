// A compiled host that records arena games and replays them through the C ABI (include/diee.hpp over include/diee.h), the way a Rust
// binding would: Random-vs-Random games with the turn log (diee_arena_ex), every game re-played turn by turn from its initial state with the
// rules entry points (diee_bg_legal_moves for the legality of each action, diee_bg_apply with the recorded dice), the last state compared
// with the call's final_states.  Build: g++ -std=c++17 -Iinclude examples/arena_replay.cpp -Ldie-e_amd -ldiee -o arena_replay
//   ./arena_replay [games=8]          exit 0: every replay ends on the game's final state, all 32 bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "diee.hpp"

int main(int argc, char** argv) {
    const uint32_t games = argc > 1 ? (uint32_t)atoi(argv[1]) : 8;
    try {
        diee_host::Engine eng(0);                                                 // (Random agents need no weights)
        const diee_host::MctsConfig cfg{8, 2.0f, 400, 0.3f, 0.25f};
        const auto r = eng.arena(nullptr, cfg, 1.25f, 0xD1EE0001ull, games, 400, DIEE_AGENT_RANDOM, DIEE_AGENT_RANDOM, 0, true, /*record_turns=*/true);
        uint32_t matching = 0;
        uint64_t skipped = 0;
        for (uint32_t g = 0; g < games; ++g) {
            diee_host::Backgammon s = r.initial_states[g];
            bool ok = true;
            for (uint64_t t = r.first[g]; t < r.first[g + 1] && ok; ++t) {
                const diee_turn& turn = r.turns[t];
                ok = turn.roll[0] == s.roll[0] && turn.roll[1] == s.roll[1] && turn.player == s.player && turn.second == s.second &&
                     turn.agent == DIEE_AGENT_RANDOM && (turn.retired != 0) == (t + 1 == r.first[g + 1] && r.retired_round[g] != UINT32_MAX);
                const auto legal = eng.get_valid_moves({s})[0];
                if (turn.play[0] == DIEE_NO_MOVE) {                               // skip_turn, backgammon_logic.rs:192-196: only without a legal play
                    ok = ok && legal.empty();
                    s.second = 0; s.player = (int8_t)-s.player; s.roll[0] = turn.next_roll[0]; s.roll[1] = turn.next_roll[1];
                    ++skipped;
                    continue;
                }
                diee_host::Play p;
                std::memcpy(p.mv, turn.play, 4);
                bool found = false;
                for (const auto& q : legal) found = found || std::memcmp(q.mv, p.mv, 4) == 0;
                ok = ok && found;
                s = eng.apply_move(s, p, turn.next_roll);
            }
            ok = ok && std::memcmp(&s, &r.final_states[g], sizeof s) == 0;
            if (!ok) std::fprintf(stderr, "game %u: the replay does not reach the final state\n", g);
            matching += ok;
        }
        std::printf("arena_replay: %u games, %llu turns (%llu skipped), %u replays reach the final state\n", games,
                    (unsigned long long)r.first[games], (unsigned long long)skipped, matching);
        return matching == games ? 0 : 2;
    } catch (const diee_host::Error& e) {
        std::fprintf(stderr, "diee error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
}
