// Stand-alone host program over csrc/prefix_classify.hpp (no HIP): T0, the
// lower bound on the time of a program image's first SEND.
// Built and run by tests/test_prefix_host.py with -fsanitize=address,undefined.
// With an argument: a program image as text (`n_insns n_consts main_pc`, then
// w0 imm per instruction, then the constants); prints its T0.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../time-warp_amd/csrc/prefix_classify.hpp"

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            return 1;                                         \
        }                                                     \
    } while (0)

static tw_insn I(uint32_t op, uint32_t a = 0, uint32_t b = 0, int32_t imm = 0) {
    return tw_insn{op | (a << 8) | (b << 16), imm};
}

static int from_file(const char* path) {
    FILE* f = fopen(path, "r");
    CHECK(f);
    unsigned n = 0, nc = 0, main_pc = 0;
    CHECK(fscanf(f, "%u %u %u", &n, &nc, &main_pc) == 3);
    std::vector<tw_insn> in(n);
    std::vector<int64_t> k(nc);
    for (unsigned i = 0; i < n; ++i) {
        unsigned w0 = 0;
        int imm = 0;
        CHECK(fscanf(f, "%u %d", &w0, &imm) == 2);
        in[i] = tw_insn{w0, imm};
    }
    for (unsigned i = 0; i < nc; ++i) CHECK(fscanf(f, "%" SCNd64, &k[i]) == 1);
    fclose(f);
    printf("t0 %" PRId64 "\n", tw::prefix_t0(in.data(), n, k.data(), nc, main_pc));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return from_file(argv[1]);
    const int64_t S1 = 1000000, S5 = 5000000;
    const int64_t K[] = {S1, S5, 250, -7};
    const uint32_t NK = 4, USER0 = TW_EXC_USER0;
    auto t0 = [&](const std::vector<tw_insn>& in, uint32_t main_pc = 0) {
        return tw::prefix_t0(in.data(), (uint32_t)in.size(), K, NK, main_pc);
    };
    // a send at t = 0; behind computation; behind a fused pair (continues at pc + 2)
    CHECK(t0({I(TW_OP_SEND), I(TW_OP_END)}) == 0);
    CHECK(t0({I(TW_OP_SETI), I(TW_OP_LINK), I(TW_OP_SEND), I(TW_OP_END)}) == 0);
    CHECK(t0({I(TW_OP_SETI, 0, TW_ALU_NSTORE), I(TW_OP_END), I(TW_OP_SEND), I(TW_OP_END)}) == 0);
    // behind WAIT_REL: its constant; a negative constant waits 0; a register wait adds nothing
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND), I(TW_OP_END)}) == S1);
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 3), I(TW_OP_SEND), I(TW_OP_END)}) == 0);
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 2), I(TW_OP_WAIT_REG, 1), I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND)}) == S1 + 250);
    // behind WAIT_ABS: max(d, K)
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 2), I(TW_OP_WAIT_ABS, 0, 0, 0), I(TW_OP_SEND), I(TW_OP_END)}) == S1);
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 1), I(TW_OP_WAIT_ABS, 0, 0, 0), I(TW_OP_SEND), I(TW_OP_END)}) == S5);
    // in a forked child: the child starts at the fork's time; main itself never sends
    CHECK(t0({I(TW_OP_FORK, 1, 0xFFFF, 3), I(TW_OP_WAIT_REL, 0, 0, 1), I(TW_OP_END),
              /* 3 */ I(TW_OP_WAIT_REL, 0, 0, 2), I(TW_OP_SEND), I(TW_OP_END)}) == 250);
    // two paths to one send: the shorter one counts, whichever the walk meets first
    CHECK(t0({I(TW_OP_JEQI, 0, 0, 3), I(TW_OP_WAIT_REL, 0, 0, 1), I(TW_OP_JMP, 0, 0, 4),
              /* 3 */ I(TW_OP_WAIT_REL, 0, 0, 2), /* 4 */ I(TW_OP_SEND), I(TW_OP_END)}) == 250);
    {
        // a send in a catch handler: main throws at t = 0 to the child, whose only
        // exception-free path to the handler passes a 1-s wait
        std::vector<tw_insn> in = {
            /* 0 */ I(TW_OP_FORK, 1, 0xFFFF, 3), I(TW_OP_THROW_TO, 1, USER0), I(TW_OP_END),
            /* 3 */ I(TW_OP_CATCH, 0, 1u << USER0, 6), I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_UNCATCH),
            /* 6 */ I(TW_OP_SEND), I(TW_OP_END),
        };
        CHECK(t0(in) == 0);
        // ... a mask that does not take the code: the handler is reached through the wait only
        in[3] = I(TW_OP_CATCH, 0, 1u << (USER0 + 1), 6);
        CHECK(t0(in) == S1);
        // ... a throwM of the code in another thread still reaches it (over-approximated)
        in[1] = I(TW_OP_THROW, 0, USER0 + 1);
        CHECK(t0(in) == 0);
        // ... thrown late: the handler no sooner than the throw
        in[0] = I(TW_OP_FORK, 1, 0xFFFF, 3);
        in[1] = I(TW_OP_THROW_TO, 1, USER0 + 1);
        in.insert(in.begin() + 1, I(TW_OP_WAIT_REL, 0, 0, 2));  // pcs shift by one
        in[0].imm = 4;
        in[4].imm = 7;
        CHECK(t0(in) == 250);
    }
    {
        // a send in a timeout's handler: no later than the timeout K = 250
        std::vector<tw_insn> in = {
            /* 0 */ I(TW_OP_CATCH, 0, 1u << TW_EXC_TIMEOUT, 6), I(TW_OP_TMO_BEGIN, 0, 0, 2), I(TW_OP_WAIT_REL, 0, 0, 1),
            /* 3 */ I(TW_OP_TMO_END), I(TW_OP_UNCATCH), I(TW_OP_END),
            /* 6 */ I(TW_OP_SEND), I(TW_OP_END),
        };
        CHECK(t0(in) <= 250);
        in[0] = I(TW_OP_CATCH, 0, 1u << TW_EXC_THREAD_KILLED, 6);  // not a handler of the timeout
        CHECK(t0(in) == INT64_MAX);
    }
    {
        // a send only in a listener's handler (entered through a delivery: no
        // entry edge) and another at 5 s
        std::vector<tw_insn> in = {
            /* 0 */ I(TW_OP_LISTEN), I(TW_OP_WAIT_REL, 0, 0, 1), I(TW_OP_SEND), I(TW_OP_END),
            /* 4: the handler */ I(TW_OP_TRACE), I(TW_OP_SEND), I(TW_OP_END),
        };
        CHECK(t0(in) == S5);
    }
    // no send at all; none that is reachable
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_END)}) == INT64_MAX);
    CHECK(t0({I(TW_OP_END), I(TW_OP_SEND)}) == INT64_MAX);
    // out of range: a constant index, a jump, a fork, a handler, the opcode, main_pc
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 99), I(TW_OP_SEND)}) == 0);
    CHECK(t0({I(TW_OP_WAIT_ABS, 0, 0, -1), I(TW_OP_SEND)}) == 0);
    CHECK(t0({I(TW_OP_JMP, 0, 0, 1000), I(TW_OP_SEND)}) == 0);
    CHECK(t0({I(TW_OP_JNEI, 0, 0, -1), I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND)}) == 0);
    CHECK(t0({I(TW_OP_FORK, 1, 0xFFFF, 7), I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND)}) == 0);
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND), I(TW_OP_END), I(TW_OP_CATCH, 0, 0xFFFE, 50)}) == 0);
    CHECK(t0({I(TW_OP_COUNT + 3), I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND)}) == 0);
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND)}, 2) == 0);
    CHECK(tw::prefix_t0(nullptr, 0, nullptr, 0, 0) == 0);
    {   // a wait with no constant pool at all
        const std::vector<tw_insn> in = {I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_SEND)};
        CHECK(tw::prefix_t0(in.data(), 2, nullptr, 0, 0) == 0);
    }
    // the walk falls off the image's end: nothing there
    CHECK(t0({I(TW_OP_WAIT_REL, 0, 0, 0), I(TW_OP_NOP)}) == INT64_MAX);
    // waits that would overflow saturate
    {
        const int64_t big[] = {INT64_MAX - 5, 100};
        const std::vector<tw_insn> in = {I(TW_OP_WAIT_ABS, 0, 0, 0), I(TW_OP_WAIT_REL, 0, 0, 1), I(TW_OP_SEND)};
        CHECK(tw::prefix_t0(in.data(), 3, big, 2, 0) == INT64_MAX);
    }
    printf("prefix ok\n");
    return 0;
}
