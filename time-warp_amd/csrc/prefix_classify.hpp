// prefix_classify.hpp — the load-time bound of the send-free prefix
// (prefix.hip): T0, a lower bound on the virtual time at which
// any thread of the program image can execute its first TW_OP_SEND.  Until
// then no replica reads its link-table column, so (with no per-replica main
// registers) every replica of the batch passes through the same states.
// Kept free of HIP so it compiles into a plain host program
// (tests/prefix_classify_main.cpp, run under ASan / UBSan).
//
// A shortest path over the image from main_pc at time 0.  Every edge function
// is monotone and never lowers the time, so Dijkstra's order holds:
//   fall-through, jumps (both arms)   d
//   FORK                              d to the child pc, d for the parent
//   WAIT_REL K[imm]                   d + max(K, 0)
//   WAIT_ABS K[imm]                   max(d, K)
//   WAIT_REG                          d   (the register is unknown: >= 0)
//   END                               none
// Exceptions are asynchronous: a THROW_TO, THROW, TMO_FIRE or TMO_BEGIN (its
// watchdog fires later still) reached at d gives d to the handler of every
// CATCH whose mask takes its code.  Finally frames (TMO_PUSH) carry no pc: an
// unwind through them continues at a CATCH handler or ends the thread.
// Listener handlers and the DELIVER stub are entered only through a delivery,
// which needs a SEND first: they get no entry edge.  The fused pairs of
// Program.finalize (TW_ALU_NSTORE, TW_TRACE_PAIR) continue at pc + 2; they
// reach pc + 1 as well (an over-approximation only lowers T0, which is safe).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "../../include/timewarp.h"

namespace tw {

// T0 of the image: the minimum of the distances of its reachable SENDs;
// INT64_MAX when no SEND is reachable; 0 (no prefix) when an instruction the
// walk reaches has a pc or a constant index out of range or an unknown opcode.
inline int64_t prefix_t0(const tw_insn* in, uint32_t n, const int64_t* consts, uint32_t n_consts, uint32_t main_pc) {
    if (!in || main_pc >= n) return 0;
    constexpr int64_t INF = INT64_MAX;
    // every CATCH of the image: handler pc and mask
    std::vector<std::pair<uint32_t, uint32_t>> handlers;
    for (uint32_t pc = 0; pc < n; ++pc) {
        if ((in[pc].w0 & 0xFFu) != TW_OP_CATCH) continue;
        if (in[pc].imm < 0 || (uint32_t)in[pc].imm >= n) return 0;
        handlers.emplace_back((uint32_t)in[pc].imm, in[pc].w0 >> 16);
    }
    std::vector<int64_t> dist(n, INF);
    using Item = std::pair<int64_t, uint32_t>;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> pq;
    auto relax = [&](uint32_t pc, int64_t d) {
        if (pc < n && d < dist[pc]) {
            dist[pc] = d;
            pq.emplace(d, pc);
        }
    };
    auto raise = [&](uint32_t code, int64_t d) {
        for (const auto& h : handlers)
            if (code == 0 || code > 15 || (h.second & (1u << code))) relax(h.first, d);
    };
    auto add = [](int64_t d, int64_t k) { return k <= 0 ? d : (d > INF - k ? INF : d + k); };
    int64_t t0 = INF;
    relax(main_pc, 0);
    while (!pq.empty()) {
        const Item it = pq.top();
        pq.pop();
        const int64_t d = it.first;
        const uint32_t pc = it.second;
        if (d != dist[pc]) continue;
        if (d >= t0) break;  // nothing earlier is left
        const uint32_t w = in[pc].w0, op = w & 0xFFu, b = w >> 16;
        const int64_t imm = in[pc].imm;
        const bool pc_ok = imm >= 0 && (uint64_t)imm < n, k_ok = consts && imm >= 0 && (uint64_t)imm < n_consts;
        switch (op) {
        case TW_OP_END:
            break;
        case TW_OP_WAIT_REL:
            if (!k_ok) return 0;
            relax(pc + 1, add(d, consts[imm]));
            break;
        case TW_OP_WAIT_ABS:
            if (!k_ok) return 0;
            relax(pc + 1, consts[imm] > d ? consts[imm] : d);
            break;
        case TW_OP_FORK:
            if (!pc_ok) return 0;
            relax((uint32_t)imm, d);
            relax(pc + 1, d);
            break;
        case TW_OP_JMP:
            if (!pc_ok) return 0;
            relax((uint32_t)imm, d);
            break;
        case TW_OP_JEQ: case TW_OP_JNE: case TW_OP_JLT: case TW_OP_JLE: case TW_OP_JEQI: case TW_OP_JNEI:
            if (!pc_ok) return 0;
            relax((uint32_t)imm, d);
            relax(pc + 1, d);
            break;
        case TW_OP_THROW_TO:
            raise(b & 0xFFu, d);
            relax(pc + 1, d);
            break;
        case TW_OP_THROW:
            raise(b & 0xFFu, d);  // (the thread itself goes on at a handler or dies)
            break;
        case TW_OP_TMO_FIRE:
        case TW_OP_TMO_BEGIN:
            if (op == TW_OP_TMO_BEGIN && !k_ok) return 0;
            raise(TW_EXC_TIMEOUT, d);
            relax(pc + 1, d);
            break;
        case TW_OP_SEND:
            t0 = d < t0 ? d : t0;
            break;
        case TW_OP_SETI: case TW_OP_SETK: case TW_OP_ADDI: case TW_OP_MULI: case TW_OP_NOW: case TW_OP_NODE:
        case TW_OP_TRACE:
            // (TW_ALU_NSTORE and TW_TRACE_PAIR are the same bit: the fused pair continues at pc + 2)
            relax(pc + 1, d);
            if (b & TW_ALU_NSTORE) relax(pc + 2, d);
            break;
        default:
            if (op >= TW_OP_COUNT) return 0;
            relax(pc + 1, d);
            break;
        }
    }
    return t0;
}

}  // namespace tw
