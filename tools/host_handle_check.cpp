// Developer tool (build container, no GPU): a device -1 handle driven through the C ABI from a program of its own, so that the host side of
// the solver handle can be run under the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-inline-asm -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/host_handle_check.cpp sig_sdp_mmw_amd/csrc/mmw_api.hip -o host_handle_check && ./host_handle_check
// Creates fp32 and fp64 handles on a two-clique state, reads every size, every int list and the three float fields a host-only handle
// answers, checks that everything that needs the device is refused with a message, and destroys the handles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mmw_hip.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { ++failures; std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, mmw_last_error()); }
}

int main() {
    // six users in two association cliques {0,1,2} and {3,4,5}; gains between the cliques, own gain on the diagonal
    const int K = 6, Z = 3;
    std::vector<int32_t> Sp{0}, Si, Qp{0}, Qi;
    std::vector<double> Sx, Qx, h(K);
    for (int a = 0; a < K; ++a) {
        for (int b = 0; b < K; ++b) {
            if (a == b) { Si.push_back(b); Sx.push_back(4.0 + a); }
            else if (a / 3 != b / 3) { Si.push_back(b); Sx.push_back(0.05 * (1 + ((a * 7 + b * 3) % 5))); }
            else { Qi.push_back(b); Qx.push_back(1.0); }
        }
        Sp.push_back((int32_t)Si.size());
        Qp.push_back((int32_t)Qi.size());
        h[a] = 1.5 + 0.25 * a;
    }
    for (int dtype : {MMW_F32, MMW_F64}) {
        mmw_solver* s = nullptr;
        expect(mmw_create(&s, -1, dtype, K, Z, 2, 0.1, 3, Sp.data(), Si.data(), Sx.data(), Qp.data(), Qi.data(), Qx.data(), h.data()) == MMW_OK && s, "mmw_create");
        if (!s) return 1;
        int64_t sz[10];
        expect(mmw_sizes(s, sz) == MMW_OK && sz[0] == K && sz[1] == Z && sz[2] == 2 * Z && sz[9] == 0, "mmw_sizes");
        const int64_t ilen[10] = {sz[0] + 1, sz[4], sz[0] + 1, sz[5], sz[6], sz[6], sz[7], sz[7], sz[0], sz[7]};
        for (int f = 0; f < 10; ++f) {
            std::vector<int32_t> v((size_t)ilen[f] + 1);
            expect(mmw_read_i32(s, f, v.data(), ilen[f]) == MMW_OK, "mmw_read_i32");
            expect(mmw_read_i32(s, f, v.data(), ilen[f] + 1) != MMW_OK, "mmw_read_i32 refuses a wrong length");
        }
        const struct { int which; int64_t n; } ff[3] = {{MMW_F_S_SUM, sz[0]}, {MMW_F_NORM_H, sz[0]}, {MMW_F_ST_DATA, sz[5]}};
        for (const auto& f : ff) {
            std::vector<double> v((size_t)f.n + 1);
            expect(mmw_read_f64(s, f.which, v.data(), f.n) == MMW_OK, "mmw_read_f64 of a host field");
        }
        double one[4];
        for (int which : {MMW_F_Y, MMW_F_LVAL, MMW_F_XAVG, MMW_F_E_MAX, MMW_F_BLOCKING})
            expect(mmw_read_f64(s, which, one, 1) != MMW_OK && std::strlen(mmw_last_error()) > 0, "mmw_read_f64 of a device field is refused");
        expect(mmw_set_slots(s, Z + 1, 3) != MMW_OK, "mmw_set_slots is refused");
        expect(mmw_set_slots_warm(s, Z + 1, 3) != MMW_OK, "mmw_set_slots_warm is refused");
        expect(mmw_reset(s, 3) != MMW_OK, "mmw_reset is refused");
        expect(mmw_iterate(s, 1, nullptr, 1) != MMW_OK, "mmw_iterate is refused");
        expect(mmw_sync(s) != MMW_OK, "mmw_sync is refused");
        expect(mmw_gap(s, one) != MMW_OK, "mmw_gap is refused");
        expect(mmw_factor(s, 2, nullptr, 0) != MMW_OK, "mmw_factor is refused");
        expect(mmw_sketch(s, 1, 0, one, 1) != MMW_OK, "mmw_sketch is refused");
        expect(mmw_set_profile(s, 1) != MMW_OK, "mmw_set_profile is refused");
        expect(mmw_bench_spmm(s, 0, 1, one) != MMW_OK, "mmw_bench_spmm is refused");
        expect(mmw_set_eta(s, 0.2) == MMW_OK, "mmw_set_eta");
        expect(mmw_set_expm(s, MMW_EXPM_LANCZOS, 8, 1e-8) == MMW_OK, "mmw_set_expm");
        expect(mmw_set_timing(s, 1) == MMW_OK, "mmw_set_timing");
        expect(mmw_destroy(s) == MMW_OK, "mmw_destroy");
    }
    // a refused creation leaves no handle behind
    mmw_solver* s = nullptr;
    expect(mmw_create(&s, -1, MMW_F64, K, 1, 2, 0.1, 3, Sp.data(), Si.data(), Sx.data(), Qp.data(), Qi.data(), Qx.data(), h.data()) != MMW_OK && !s, "mmw_create refuses Z = 1");
    std::printf("host_handle_check: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
