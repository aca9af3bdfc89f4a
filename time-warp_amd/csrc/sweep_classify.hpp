// sweep_classify.hpp — the load-time classifier of the killThread sweep
// (sweep.hip): which resume pcs are kill-stub entries, and at
// which absolute times the program image parks threads in front of them.
// Kept free of HIP so it compiles into a plain host program
// (tests/sweep_classify_main.cpp, run under ASan / UBSan).
//
// A kill stub is `THROW_TO ra, ThreadKilled [; THROW_TO rb, ThreadKilled] ; END`
// (`mapM_ killThread [r1, r2]`, examples/token-ring/Main.hs:124-127).  A resume
// pc is a kill-stub ENTRY when its code is that sequence itself or an
// unconditional JMP to it (`schedule t act` = `wait t ; jmp act`, program.py
// Code.schedule).  A SWEEP TIME is the constant of a `WAIT_ABS K[imm]` whose
// next instruction is such an entry: the wake time of every thread parked there.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/timewarp.h"

namespace tw {

#define TW_SWEEP_MAX_TIMES 4u  // more distinct sweep times than this: no sweeping

// the stub word of a resume pc (0: not a kill-stub entry)
#define SWB_VALID 1u
#define SWB_TWO 2u                             // two throwTos
#define SWB_RA0(w) (((w) >> 2) & 3u)           // the first ref's register
#define SWB_RA1(w) (((w) >> 4) & 3u)           // the second's

struct SweepPlan {
    std::vector<uint32_t> stub;   // [n_insns + 1] stub words (entry n_insns: 0)
    std::vector<int64_t> times;   // distinct sweep times, ascending; empty: no sweeping
    uint32_t n_stub_pcs = 0;
};

// the stub word of the sequence starting at q (0: none)
inline uint32_t sweep_seq_word(const tw_insn* in, uint32_t n, uint32_t q) {
    auto op = [&](uint32_t i) { return i < n ? in[i].w0 & 0xFFu : (uint32_t)TW_OP_NOP; };
    auto kill = [&](uint32_t i) { return op(i) == TW_OP_THROW_TO && ((in[i].w0 >> 16) & 0xFFu) == TW_EXC_THREAD_KILLED; };
    if (q >= n || !kill(q)) return 0u;
    const uint32_t ra0 = (in[q].w0 >> 8) & 3u;
    if (op(q + 1) == TW_OP_END) return SWB_VALID | (ra0 << 2);
    if (q + 1 < n && kill(q + 1) && op(q + 2) == TW_OP_END)
        return SWB_VALID | SWB_TWO | (ra0 << 2) | (((in[q + 1].w0 >> 8) & 3u) << 4);
    return 0u;
}

inline SweepPlan sweep_classify(const tw_insn* in, uint32_t n, const int64_t* consts, uint32_t n_consts) {
    SweepPlan p;
    p.stub.assign((size_t)n + 1, 0u);
    if (!in) return p;
    for (uint32_t pc = 0; pc < n; ++pc) {
        uint32_t q = pc;
        if ((in[pc].w0 & 0xFFu) == TW_OP_JMP) {
            if (in[pc].imm < 0 || (uint32_t)in[pc].imm >= n) continue;
            q = (uint32_t)in[pc].imm;
        }
        p.stub[pc] = sweep_seq_word(in, n, q);
        p.n_stub_pcs += p.stub[pc] ? 1u : 0u;
    }
    bool over = false;
    for (uint32_t pc = 0; pc + 1 < n && !over; ++pc) {
        if ((in[pc].w0 & 0xFFu) != TW_OP_WAIT_ABS || !p.stub[pc + 1]) continue;
        if (!consts || in[pc].imm < 0 || (uint32_t)in[pc].imm >= n_consts) continue;
        const int64_t t = consts[in[pc].imm];
        size_t i = 0;
        while (i < p.times.size() && p.times[i] < t) ++i;
        if (i < p.times.size() && p.times[i] == t) continue;
        if (p.times.size() == TW_SWEEP_MAX_TIMES) { over = true; break; }
        p.times.insert(p.times.begin() + (ptrdiff_t)i, t);
    }
    if (over) p.times.clear();
    return p;
}

}  // namespace tw
