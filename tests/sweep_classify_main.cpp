// Stand-alone host program over csrc/sweep_classify.hpp (no HIP): which resume
// pcs are kill-stub entries and which WAIT_ABS constants are sweep times.
// Built and run by tests/test_sweep_host.py with -fsanitize=address,undefined.
// With an argument: a program image as text (`n_insns n_consts`, then w0 imm
// per instruction, then the constants); prints its stub pcs and sweep times.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../time-warp_amd/csrc/sweep_classify.hpp"

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
static tw_insn KILL(uint32_t ra) { return I(TW_OP_THROW_TO, ra, TW_EXC_THREAD_KILLED); }

static int from_file(const char* path) {
    FILE* f = fopen(path, "r");
    CHECK(f);
    unsigned n = 0, nc = 0;
    CHECK(fscanf(f, "%u %u", &n, &nc) == 2);
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
    const tw::SweepPlan p = tw::sweep_classify(in.data(), n, k.data(), nc);
    CHECK(p.stub.size() == (size_t)n + 1 && p.stub[n] == 0);
    printf("stubs");
    for (unsigned i = 0; i < n; ++i)
        if (p.stub[i]) printf(" %u:%u:%u:%u", i, (p.stub[i] & SWB_TWO) ? 2u : 1u, SWB_RA0(p.stub[i]), SWB_RA1(p.stub[i]));
    printf("\ntimes");
    for (int64_t t : p.times) printf(" %" PRId64, t);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return from_file(argv[1]);
    const int64_t K[] = {100, 200, 300, 400, 500, 100};
    {
        // stubs of 0, 1, 2 and 3 throwTos, each behind `WAIT_ABS ; JMP`
        std::vector<tw_insn> in = {
            /* 0 */ I(TW_OP_WAIT_ABS, 0, 0, 0), I(TW_OP_JMP, 0, 0, 8),    // -> 0 throwTos
            /* 2 */ I(TW_OP_WAIT_ABS, 0, 0, 1), I(TW_OP_JMP, 0, 0, 9),    // -> 1
            /* 4 */ I(TW_OP_WAIT_ABS, 0, 0, 2), I(TW_OP_JMP, 0, 0, 11),   // -> 2
            /* 6 */ I(TW_OP_WAIT_ABS, 0, 0, 3), I(TW_OP_JMP, 0, 0, 14),   // -> 3
            /* 8 */ I(TW_OP_END),
            /* 9 */ KILL(1), I(TW_OP_END),
            /* 11 */ KILL(1), KILL(2), I(TW_OP_END),
            /* 14 */ KILL(1), KILL(2), KILL(3), I(TW_OP_END),
        };
        const uint32_t n = (uint32_t)in.size();
        const tw::SweepPlan p = tw::sweep_classify(in.data(), n, K, 6);
        CHECK(p.stub.size() == n + 1);
        CHECK(p.stub[1] == 0 && p.stub[8] == 0);                       // plain END: not a stub
        CHECK(p.stub[3] == (SWB_VALID | (1u << 2)) && p.stub[9] == p.stub[3]);
        CHECK(p.stub[5] == (SWB_VALID | SWB_TWO | (1u << 2) | (2u << 4)) && p.stub[11] == p.stub[5]);
        CHECK(p.stub[12] == (SWB_VALID | (2u << 2)));                  // the pair's second throwTo: a stub of one
        CHECK(p.stub[7] == 0 && p.stub[14] == 0);                      // three: not a stub
        CHECK(p.stub[15] == (SWB_VALID | SWB_TWO | (2u << 2) | (3u << 4)));  // ... but its last two are
        CHECK(p.stub[n] == 0);
        CHECK(p.times.size() == 2 && p.times[0] == 200 && p.times[1] == 300);
    }
    {
        // a stub reached by a conditional jump, a register wait, another exception code
        std::vector<tw_insn> in = {
            /* 0 */ I(TW_OP_WAIT_ABS, 0, 0, 0), I(TW_OP_JEQI, 0, 0, 6),  // conditional: no entry, no sweep time
            /* 2 */ I(TW_OP_WAIT_REG, 1), I(TW_OP_JMP, 0, 0, 6),         // entry, but the wait has no constant
            /* 4 */ I(TW_OP_WAIT_ABS, 0, 0, 1), I(TW_OP_JMP, 0, 0, 8),   // throwTo of another code: no stub
            /* 6 */ KILL(1), I(TW_OP_END),
            /* 8 */ I(TW_OP_THROW_TO, 1, TW_EXC_TIMEOUT), I(TW_OP_END),
            /* 10 */ I(TW_OP_WAIT_ABS, 0, 0, 99), I(TW_OP_JMP, 0, 0, 6), // constant index out of range: ignored
            /* 12 */ I(TW_OP_JMP, 0, 0, 1000), I(TW_OP_JMP, 0, 0, -1),   // jumps out of the image
        };
        const uint32_t n = (uint32_t)in.size();
        const tw::SweepPlan p = tw::sweep_classify(in.data(), n, K, 6);
        CHECK(p.stub[1] == 0 && p.stub[3] != 0 && p.stub[6] != 0 && p.stub[5] == 0 && p.stub[8] == 0);
        CHECK(p.stub[11] != 0 && p.stub[12] == 0 && p.stub[13] == 0);
        CHECK(p.times.empty());
    }
    {
        // sweep times: duplicates count once; more distinct ones than the cap: none
        for (uint32_t waits = 1; waits <= 6; ++waits) {
            std::vector<tw_insn> in;
            for (uint32_t i = 0; i < waits; ++i) {
                in.push_back(I(TW_OP_WAIT_ABS, 0, 0, (int32_t)(waits - 1 - i)));  // descending constants
                in.push_back(I(TW_OP_JMP, 0, 0, (int32_t)(2 * waits)));
            }
            in.push_back(KILL(1));
            in.push_back(I(TW_OP_END));
            const tw::SweepPlan p = tw::sweep_classify(in.data(), (uint32_t)in.size(), K, 6);
            // K[5] == K[0]: six waits name five distinct times
            const uint32_t distinct = waits == 6 ? 5 : waits;
            if (distinct <= TW_SWEEP_MAX_TIMES) {
                CHECK(p.times.size() == distinct);
                for (size_t i = 0; i + 1 < p.times.size(); ++i) CHECK(p.times[i] < p.times[i + 1]);
            } else {
                CHECK(p.times.empty());
            }
            CHECK(p.n_stub_pcs == waits + 1);
        }
    }
    {
        // an empty image, a missing constant pool, a stub cut off by the image's end
        const tw::SweepPlan e = tw::sweep_classify(nullptr, 0, nullptr, 0);
        CHECK(e.stub.size() == 1 && e.times.empty());
        std::vector<tw_insn> in = {I(TW_OP_WAIT_ABS, 0, 0, 0), KILL(1), KILL(2)};
        const tw::SweepPlan p = tw::sweep_classify(in.data(), 3, nullptr, 0);
        CHECK(p.stub[1] == 0 && p.stub[2] == 0 && p.times.empty());
    }
    printf("classify ok\n");
    return 0;
}
