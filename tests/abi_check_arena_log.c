/* Compiled as C11 by tests/test_arena_log_cpu.py (gcc -std=c11 -Iinclude): the three structs of diee_arena_ex -- the turn record, the
 * log and the options -- as a Rust #[repr(C)] binding sees them, asserted at compile time and printed for the comparison with the ctypes
 * mirrors in die-e_amd/__init__.py. */
#include <stddef.h>
#include <stdio.h>
#include "diee.h"

_Static_assert(sizeof(diee_turn) == 12, "diee_turn is 12 bytes");
_Static_assert(offsetof(diee_turn, play) == 0 && offsetof(diee_turn, roll) == 4 && offsetof(diee_turn, next_roll) == 6 &&
               offsetof(diee_turn, player) == 8 && offsetof(diee_turn, agent) == 9 && offsetof(diee_turn, second) == 10 &&
               offsetof(diee_turn, retired) == 11, "diee_turn fields");
_Static_assert(sizeof(diee_arena_log) == 4 * sizeof(void*), "diee_arena_log");
_Static_assert(sizeof(diee_arena_opts) == 16 + sizeof(void*) && offsetof(diee_arena_opts, flags) == 4 && offsetof(diee_arena_opts, log) == 16,
               "diee_arena_opts");

#define F(T, f) printf("  \"%s.%s\": %zu,\n", #T, #f, offsetof(T, f))
int main(void) {
    printf("{\n");
    F(diee_turn, play); F(diee_turn, roll); F(diee_turn, next_roll); F(diee_turn, player); F(diee_turn, agent); F(diee_turn, second);
    F(diee_turn, retired);
    F(diee_arena_log, turns); F(diee_arena_log, first); F(diee_arena_log, n_games); F(diee_arena_log, owner);
    F(diee_arena_opts, struct_size); F(diee_arena_opts, flags); F(diee_arena_opts, log);
    printf("  \"sizeof.diee_turn\": %zu, \"sizeof.diee_arena_log\": %zu, \"sizeof.diee_arena_opts\": %zu\n}\n", sizeof(diee_turn),
           sizeof(diee_arena_log), sizeof(diee_arena_opts));
    return 0;
}
