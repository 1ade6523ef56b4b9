// Developer tool (build container, no GPU): every refusal of mmw_factor_random that the host can reach, on device -1 solver handles, driven
// through the C ABI from a program of its own so that the entry's host side can be run under the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-inline-asm -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/host_factor_random_check.cpp sig_sdp_mmw_amd/csrc/mmw_api.hip -o host_factor_random_check && ./host_factor_random_check
// Handles of several sizes and both dtypes; for each: the null handle, cols < 1, index_order outside {0, 1}, a width past
// MMW_FACTOR_RANDOM_MAX_COLS, and what is in range (MMW_ERR_STATE: a host-only handle has nowhere to draw) -- each with the status, a
// message that names the offending value, and a guarded output buffer that must come back untouched.  Afterwards the handle still answers
// mmw_sizes and refuses mmw_round's resident factor (none was made).  The sibling of tools/host_carry_check.cpp.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mmw_hip.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { ++failures; std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, mmw_last_error()); }
}
static bool says(const std::string& part) { return std::string(mmw_last_error()).find(part) != std::string::npos; }

struct State {
    int K;
    std::vector<int32_t> Sp{0}, Si, Qp{0}, Qi;
    std::vector<double> Sx, Qx, h;
    // K users in two association cliques; gains between the cliques, own gain on the diagonal
    explicit State(int K_) : K(K_), h((size_t)K_) {
        const int half = K / 2;
        for (int a = 0; a < K; ++a) {
            for (int b = 0; b < K; ++b) {
                if (a == b) { Si.push_back(b); Sx.push_back(4.0 + a); }
                else if ((a < half) != (b < half)) { Si.push_back(b); Sx.push_back(0.05 * (1 + ((a * 7 + b * 3) % 5))); }
                else { Qi.push_back(b); Qx.push_back(1.0); }
            }
            Sp.push_back((int32_t)Si.size());
            Qp.push_back((int32_t)Qi.size());
            h[a] = 1.5 + 0.25 * a;
        }
    }
};

int main() {
    expect(mmw_factor_random(nullptr, 4, 0, nullptr, 1) == MMW_ERR_ARG && says("mmw_factor_random: null solver handle"), "null handle");
    for (int dtype : {MMW_F32, MMW_F64})
        for (int K : {4, 7, 24, 61}) {
            State st(K);
            mmw_solver* s = nullptr;
            expect(mmw_create(&s, -1, dtype, st.K, 3, 2, 0.05, 3, st.Sp.data(), st.Si.data(), st.Sx.data(), st.Qp.data(), st.Qi.data(), st.Qx.data(), st.h.data()) == MMW_OK,
                   "mmw_create");
            if (!s) continue;
            std::vector<double> out((size_t)K * 6, 7.0);  // K x 6: what the widest accepted call below would write
            for (int32_t cols : {0, -1, INT32_MIN}) {
                expect(mmw_factor_random(s, cols, 0, out.data(), 1) == MMW_ERR_ARG, "cols < 1");
                expect(says("cols = " + std::to_string(cols) + " must be >= 1"), "cols < 1 names the value");
            }
            for (int32_t io : {2, -1, 256, INT32_MAX}) {
                expect(mmw_factor_random(s, 6, io, out.data(), 1) == MMW_ERR_ARG, "index_order outside {0, 1}");
                expect(says("index_order = " + std::to_string(io) + " must be 0 or 1"), "index_order names the value");
            }
            for (int32_t cols : {MMW_FACTOR_RANDOM_MAX_COLS + 1, INT32_MAX}) {
                expect(mmw_factor_random(s, cols, 1, nullptr, 1) == MMW_ERR_ARG, "a width past the limit");
                expect(says("cols = " + std::to_string(cols) + " exceeds " + std::to_string(MMW_FACTOR_RANDOM_MAX_COLS)), "the width names the value and the limit");
            }
            for (int32_t io : {0, 1}) {
                expect(mmw_factor_random(s, 6, io, out.data(), ~0ull) == MMW_ERR_STATE && says("host-only"), "a host-only handle");
                expect(mmw_factor_random(s, 1, io, nullptr, 0) == MMW_ERR_STATE, "a host-only handle, one column, no output");
                expect(mmw_factor_random(s, MMW_FACTOR_RANDOM_MAX_COLS, io, nullptr, 5) == MMW_ERR_STATE, "a host-only handle at the widest width");
            }
            for (double v : out) if (v != 7.0) { expect(false, "a refused call wrote to its output"); break; }
            int64_t sz[10] = {0};
            expect(mmw_sizes(s, sz) == MMW_OK && sz[0] == K, "the handle lives on");
            std::vector<double> rv(3 * 6, 0.5);
            std::vector<int32_t> z((size_t)K), rem(1);
            expect(mmw_round(s, 3, 6, nullptr, 1, rv.data(), z.data(), rem.data()) == MMW_ERR_STATE, "mmw_round on a host-only handle");
            expect(mmw_destroy(s) == MMW_OK, "mmw_destroy");
        }
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("host_factor_random_check: ok\n");
    return 0;
}
