// Developer tool (build container, no GPU): a device -1 batch driven through the C ABI from a program of its own, so that the host side
// of a batch -- the per-instance state processing and BatchCore's offset computation, which creation and every slot change share --
// can be run under the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-inline-asm -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/host_batch_check.cpp sig_sdp_mmw_amd/csrc/mmw_api.hip -o host_batch_check && ./host_batch_check
// Creates batches of one to five two-clique states of different sizes at several slot counts, reads every size and every int list, and
// checks that what needs the device (both slot changes, reset, iterate) is refused with a message.  A second leg builds two batches of
// the same users on different states (the cliques cut at another user), asks mmw_batch_carry_map for every instance's maps both ways,
// checks them entry by entry against a search of the other batch's lists, and runs the refusals a host-only pair can reach.
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
    // (shift: the cliques are cut at another user; thin: only every thin-th gain edge is kept, so the L patterns differ too)
    explicit State(int K_, int shift = 0, int thin = 1) : K(K_), h((size_t)K_) {
        const int half = K / 2;
        auto side = [&](int a) { return (a + shift) % K < half; };
        for (int a = 0; a < K; ++a) {
            for (int b = 0; b < K; ++b) {
                if (a == b) { Si.push_back(b); Sx.push_back(4.0 + a); }
                else if (side(a) != side(b)) {
                    if ((a + b + shift) % thin) continue;
                    Si.push_back(b); Sx.push_back(0.05 * (1 + ((a * 7 + b * 3) % 5)));
                }
                else { Qi.push_back(b); Qx.push_back(1.0); }
            }
            Sp.push_back((int32_t)Si.size());
            Qp.push_back((int32_t)Qi.size());
            h[a] = 1.5 + 0.25 * a;
        }
    }
};

struct Lists {
    std::vector<int32_t> indptr, indices, ax, ay;
    int64_t K = 0, C = 0;
};
static Lists lists_of(mmw_batch* bt, int b) {
    Lists l;
    int64_t sz[10];
    expect(mmw_batch_sizes(bt, b, sz) == MMW_OK, "mmw_batch_sizes");
    l.K = sz[0]; l.C = sz[8];
    l.indptr.resize((size_t)sz[0] + 1); l.indices.resize((size_t)sz[4]); l.ax.resize((size_t)sz[7]); l.ay.resize((size_t)sz[7]);
    expect(mmw_batch_read_i32(bt, b, MMW_I_L_INDPTR, l.indptr.data(), sz[0] + 1) == MMW_OK, "read l_indptr");
    expect(mmw_batch_read_i32(bt, b, MMW_I_L_INDICES, l.indices.data(), sz[4]) == MMW_OK, "read l_indices");
    expect(mmw_batch_read_i32(bt, b, MMW_I_ASSO_X, l.ax.data(), sz[7]) == MMW_OK, "read asso_x");
    expect(mmw_batch_read_i32(bt, b, MMW_I_ASSO_Y, l.ay.data(), sz[7]) == MMW_OK, "read asso_y");
    return l;
}
// the maps of instance b of `dst` from `src`, every entry against a linear search of src's lists
static void check_maps(mmw_batch* dst, mmw_batch* src, int b) {
    const Lists n = lists_of(dst, b), o = lists_of(src, b);
    std::vector<int32_t> lmap(n.indices.size() + 1, 7), cmap((size_t)n.C + 1, 7);
    expect(mmw_batch_carry_map(dst, src, b, lmap.data(), (int64_t)n.indices.size(), cmap.data(), n.C) == MMW_OK, "mmw_batch_carry_map");
    expect(lmap.back() == 7 && cmap.back() == 7, "mmw_batch_carry_map writes its lengths and no more");
    int64_t kept = 0;
    for (int64_t a = 0; a < n.K; ++a)
        for (int32_t e = n.indptr[a]; e < n.indptr[a + 1]; ++e) {
            int32_t want = -1;
            for (int32_t j = o.indptr[a]; j < o.indptr[a + 1]; ++j)
                if (o.indices[j] == n.indices[e]) want = j;
            expect(lmap[e] == want, "lmap entry");
            kept += want >= 0;
        }
    expect(kept >= n.K, "the diagonal always carries");
    const int64_t En = (int64_t)n.ax.size(), Eo = (int64_t)o.ax.size();
    for (int64_t k = 0; k < n.K; ++k) expect(cmap[k] == k && cmap[n.K + En + k] == o.K + Eo + k, "D- and H-part by user");
    for (int64_t e = 0; e < En; ++e) {
        int64_t want = -1;
        for (int64_t j = 0; j < Eo; ++j)
            if (o.ax[j] == n.ax[e] && o.ay[j] == n.ay[e]) want = o.K + j;
        expect(cmap[n.K + e] == want, "F-part by pair");
    }
}
static mmw_batch* make(const std::vector<const State*>& st, int Z0) {
    const int B = (int)st.size();
    std::vector<int32_t> K(B), Z(B), nit(B, 3);
    std::vector<const int32_t*> sp(B), si(B), qp(B), qi(B);
    std::vector<const double*> sx(B), qx(B), hm(B);
    for (int b = 0; b < B; ++b) {
        const State& s = *st[b];
        K[b] = s.K; Z[b] = Z0 + b;
        sp[b] = s.Sp.data(); si[b] = s.Si.data(); sx[b] = s.Sx.data(); qp[b] = s.Qp.data(); qi[b] = s.Qi.data(); qx[b] = s.Qx.data(); hm[b] = s.h.data();
    }
    mmw_batch* bt = nullptr;
    expect(mmw_batch_create(&bt, -1, B, K.data(), Z.data(), 2, 0.1, nit.data(), sp.data(), si.data(), sx.data(), qp.data(), qi.data(), qx.data(), hm.data()) == MMW_OK && bt,
           "mmw_batch_create");
    return bt;
}
static int carry_leg() {
    const State a0(6), a1(6, 1, 2), b0(33), b1(33, 5, 3), c0(64), c1(64, 0, 1), d0(9), d1(7);
    mmw_batch* src = make({&a0, &b0, &c0, &d0}, 2);
    mmw_batch* dst = make({&a1, &b1, &c1, &d1}, 3);
    mmw_batch* two = make({&a1, &b1}, 3);
    if (!src || !dst || !two) return 1;
    for (int b = 0; b < 3; ++b) {
        check_maps(dst, src, b);
        check_maps(src, dst, b);
    }
    check_maps(two, src, 1);  // (the maps look at one instance: another B does not matter to them)
    int32_t one = 7;
    expect(mmw_batch_carry_map(dst, src, 3, &one, 1, &one, 1) == MMW_ERR_ARG && std::strstr(mmw_last_error(), "instance 3: K = 7 here, K = 9"), "carry_map refuses another K");
    expect(mmw_batch_carry_map(dst, src, 4, &one, 1, &one, 1) == MMW_ERR_ARG, "carry_map refuses an index out of range");
    expect(mmw_batch_carry_map(dst, src, 0, &one, 1, &one, 1) == MMW_ERR_ARG && std::strstr(mmw_last_error(), "wrong lengths"), "carry_map refuses wrong lengths");
    expect(mmw_batch_carry_map(dst, nullptr, 0, &one, 1, &one, 1) == MMW_ERR_ARG, "carry_map refuses a null batch");
    expect(one == 7, "a refused carry_map writes nothing");
    expect(mmw_batch_carry(dst, dst, nullptr) == MMW_ERR_ARG && std::strstr(mmw_last_error(), "itself"), "mmw_batch_carry refuses dst == src");
    expect(mmw_batch_carry(dst, src, nullptr) == MMW_ERR_STATE && std::strstr(mmw_last_error(), "host-only"), "mmw_batch_carry refuses host-only batches");
    const int32_t take[4] = {1, 0, 0, 0};
    expect(mmw_batch_carry(dst, src, take) == MMW_ERR_STATE, "mmw_batch_carry refuses host-only batches under take");
    expect(mmw_batch_carry(nullptr, src, nullptr) == MMW_ERR_ARG, "mmw_batch_carry refuses a null batch");
    for (mmw_batch* bt : {src, dst, two}) expect(mmw_batch_destroy(bt) == MMW_OK, "mmw_batch_destroy");
    return 0;
}

int main() {
    if (carry_leg()) return 1;
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
