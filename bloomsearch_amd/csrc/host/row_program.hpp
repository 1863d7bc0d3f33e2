// row_program.hpp — the evaluator of a row matcher's lowered program, free of any device type: evalMatcherNode over satisfaction
// flags (match.hip.h, match_lookup.hip.h).  A program is a postfix sequence of u32 ops, opcode in the top four bits:
//   TERM c (0 | c)  push flag c      AND2 (1) / OR2 (2)  pop two, push one      TRUE (3) / FALSE (4)  push the constant
// The host lowers every expression to depth <= 64 (match_api.inc lower_programs), so the stack is ONE bit per level in a u64: a lane
// evaluates over its own row's flags while the program words stay wave-uniform.  The empty program is the nil expression, which
// matches every row.  The function is constexpr: k_eval_row_programs and k_eval_row_programs_w call it with the program in the
// constant address space and their own way of reading a flag.  The walkers' epilogues (match.hip.h match_rows_body) hold the same
// loop written out, twice: called from there the function re-schedules the walk (profiles/walker_refactor.txt); the pointer type is
// a parameter so that an LDS program fits as well.  tests/row_program_check.cpp runs it on the CPU (tests/test_row_program.py).
#pragma once
#include <cstdint>

namespace bsh_prog {

constexpr uint32_t kOpTerm = 0, kOpAnd2 = 1, kOpTrue = 3, kOpFalse = 4;   // anything else: OR2 (2)
constexpr uint32_t kTermMask = 0x0FFFFFFFu;

// ops [j0, j1) of prog; term(c) -> flag c of the row, asked in program order
template <class PROG, class TERM>
constexpr bool eval_program(PROG prog, uint32_t j0, uint32_t j1, TERM &&term)
{
    uint64_t stk = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t op = prog[j], opc = op >> 28;
        if (opc == kOpTerm) stk = (stk << 1) | (uint64_t)term(op & kTermMask);
        else if (opc == kOpTrue) stk = (stk << 1) | 1ULL;
        else if (opc == kOpFalse) stk = stk << 1;
        else {
            const uint64_t x = stk & 1ULL, y = (stk >> 1) & 1ULL;
            stk = ((stk >> 2) << 1) | (opc == kOpAnd2 ? (x & y) : (x | y));
        }
    }
    return j0 == j1 ? true : (stk & 1ULL) != 0;
}

}  // namespace bsh_prog
