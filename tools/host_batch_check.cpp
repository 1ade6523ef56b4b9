// Developer tool (build container, no GPU): a device -1 batch driven through the C ABI from a program of its own, so that the host side
// of a batch -- the per-instance state processing and BatchCore's offset computation, which creation and every slot change share --
// can be run under the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-inline-asm -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/host_batch_check.cpp sig_sdp_mmw_amd/csrc/mmw_api.hip -o host_batch_check && ./host_batch_check
// Creates batches of one to five two-clique states of different sizes at several slot counts, reads every size and every int list, and
// checks that what needs the device (both slot changes, reset, iterate) is refused with a message.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mmw_hip.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { ++failures; std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, mmw_last_error()); }
}

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
    std::vector<State> pool;
    for (int K : {6, 9, 33, 64, 7}) pool.emplace_back(K);
    for (int B = 1; B <= (int)pool.size(); ++B) {
        for (int zadd : {0, 1, 5}) {
            std::vector<int32_t> K(B), Z(B), nit(B, 3);
            std::vector<const int32_t*> sp(B), si(B), qp(B), qi(B);
            std::vector<const double*> sx(B), qx(B), hm(B);
            for (int b = 0; b < B; ++b) {
                const State& s = pool[b];
                K[b] = s.K; Z[b] = 2 + zadd + b;
                sp[b] = s.Sp.data(); si[b] = s.Si.data(); sx[b] = s.Sx.data(); qp[b] = s.Qp.data(); qi[b] = s.Qi.data(); qx[b] = s.Qx.data(); hm[b] = s.h.data();
            }
            mmw_batch* bt = nullptr;
            expect(mmw_batch_create(&bt, -1, B, K.data(), Z.data(), 2, 0.1, nit.data(), sp.data(), si.data(), sx.data(), qp.data(), qi.data(), qx.data(), hm.data()) == MMW_OK && bt,
                   "mmw_batch_create");
            if (!bt) return 1;
            for (int b = 0; b < B; ++b) {
                int64_t sz[10];
                expect(mmw_batch_sizes(bt, b, sz) == MMW_OK && sz[0] == K[b] && sz[1] == Z[b] && sz[2] == 2 * Z[b] && sz[9] == 0, "mmw_batch_sizes");
                const int64_t ilen[10] = {sz[0] + 1, sz[4], sz[0] + 1, sz[5], sz[6], sz[6], sz[7], sz[7], sz[0], sz[7]};
                for (int f = 0; f < 10; ++f) {
                    std::vector<int32_t> v((size_t)ilen[f] + 1);
                    expect(mmw_batch_read_i32(bt, b, f, v.data(), ilen[f]) == MMW_OK, "mmw_batch_read_i32");
                }
                std::vector<double> v((size_t)sz[0]);
                expect(mmw_batch_read_f64(bt, b, MMW_F_NORM_H, v.data(), sz[0]) == MMW_OK, "mmw_batch_read_f64 of a host field");
                expect(mmw_batch_read_f64(bt, b, MMW_F_Y, v.data(), 1) != MMW_OK, "mmw_batch_read_f64 of a device field is refused");
            }
            expect(mmw_batch_sizes(bt, B, nullptr) != MMW_OK, "mmw_batch_sizes refuses an index out of range");
            std::vector<int32_t> Z2(Z);
            for (int b = 0; b < B; ++b) Z2[b] += (b & 1) ? 1 : -1 + 2 * (Z[b] == 2);
            expect(mmw_batch_set_slots(bt, Z2.data(), 3) != MMW_OK && std::strlen(mmw_last_error()) > 0, "mmw_batch_set_slots is refused");
            expect(mmw_batch_set_slots_warm(bt, Z2.data(), 3) != MMW_OK && std::strlen(mmw_last_error()) > 0, "mmw_batch_set_slots_warm is refused");
            expect(mmw_batch_reset(bt, 3) != MMW_OK, "mmw_batch_reset is refused");
            std::vector<uint64_t> seeds((size_t)B, 1);
            expect(mmw_batch_iterate(bt, 1, nullptr, seeds.data()) != MMW_OK, "mmw_batch_iterate is refused");
            expect(mmw_batch_destroy(bt) == MMW_OK, "mmw_batch_destroy");
        }
    }
    std::printf("host_batch_check: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
