// Developer tool (build container, no GPU): mmw_carry_map and the refusals of mmw_carry on device -1 solver handles, driven through the C
// ABI from a program of its own, so that the host merge (carry_maps, pattern.h) can be run under the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-inline-asm -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/host_carry_check.cpp sig_sdp_mmw_amd/csrc/mmw_api.hip -o host_carry_check && ./host_carry_check
// Two handles of the same users on different states (two association cliques cut at another user, the gain edges thinned differently, so
// the L patterns and the pairs both differ), at several sizes and both dtypes: the maps both ways, entry by entry against a search of the
// other handle's lists; then the refusals a host-only pair can reach.  The sibling of tools/host_batch_check.cpp.
#include <cstdio>
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

struct Handle {
    mmw_solver* s = nullptr;
    int64_t sz[10] = {0};
    std::vector<int32_t> indptr, indices, ax, ay;
    Handle(const State& st, int dtype, int Z) {
        expect(mmw_create(&s, -1, dtype, st.K, Z, 2, 0.05, 3, st.Sp.data(), st.Si.data(), st.Sx.data(), st.Qp.data(), st.Qi.data(), st.Qx.data(), st.h.data()) == MMW_OK, "mmw_create");
        if (!s) return;
        expect(mmw_sizes(s, sz) == MMW_OK, "mmw_sizes");
        indptr.resize((size_t)sz[0] + 1); indices.resize((size_t)sz[4]); ax.resize((size_t)sz[7]); ay.resize((size_t)sz[7]);
        expect(mmw_read_i32(s, MMW_I_L_INDPTR, indptr.data(), sz[0] + 1) == MMW_OK, "read l_indptr");
        expect(mmw_read_i32(s, MMW_I_L_INDICES, indices.data(), sz[4]) == MMW_OK, "read l_indices");
        expect(mmw_read_i32(s, MMW_I_ASSO_X, ax.data(), sz[7]) == MMW_OK, "read asso_x");
        expect(mmw_read_i32(s, MMW_I_ASSO_Y, ay.data(), sz[7]) == MMW_OK, "read asso_y");
    }
    ~Handle() { mmw_destroy(s); }
};

static void check_maps(Handle& d, Handle& o) {
    const int64_t K = d.sz[0], nl = d.sz[4], nc = d.sz[8], En = d.sz[7], Eo = o.sz[7];
    std::vector<int32_t> lmap((size_t)nl, 12345), cmap((size_t)nc, 12345);
    expect(mmw_carry_map(d.s, o.s, lmap.data(), nl, cmap.data(), nc) == MMW_OK, "mmw_carry_map");
    int64_t absent = 0;
    for (int64_t a = 0; a < K; ++a)
        for (int32_t e = d.indptr[a]; e < d.indptr[a + 1]; ++e) {
            int32_t want = -1;
            for (int32_t j = o.indptr[a]; j < o.indptr[a + 1]; ++j)
                if (o.indices[j] == d.indices[e]) want = j;
            expect(lmap[e] == want, "lmap entry");
            absent += want < 0;
        }
    for (int64_t k = 0; k < K; ++k) expect(cmap[k] == k && cmap[K + En + k] == K + Eo + k, "cmap D / H part");
    for (int64_t e = 0; e < En; ++e) {
        int32_t want = -1;
        for (int64_t j = 0; j < Eo; ++j)
            if (o.ax[j] == d.ax[e] && o.ay[j] == d.ay[e]) want = (int32_t)(K + j);
        expect(cmap[K + e] == want, "cmap F part");
        absent += want < 0;
    }
    expect(absent > 0, "the two states differ in entries or pairs");
    // wrong lengths: refused, nothing written
    std::vector<int32_t> guard((size_t)nl + 1, 777);
    expect(mmw_carry_map(d.s, o.s, guard.data(), nl + 1, cmap.data(), nc) == MMW_ERR_ARG && guard[0] == 777 && guard[(size_t)nl] == 777, "wrong length refused");
}

int main() {
    for (int dtype : {MMW_F32, MMW_F64})
        for (int K : {4, 7, 24, 61}) {
            State a(K, 0, 1), b(K, 1 + K / 5, 2);
            Handle ha(a, dtype, 3), hb(b, dtype, 5);
            if (!ha.s || !hb.s) continue;
            check_maps(hb, ha);
            check_maps(ha, hb);
            expect(mmw_carry(hb.s, ha.s) == MMW_ERR_STATE, "mmw_carry on host-only handles");
            expect(mmw_carry(hb.s, hb.s) == MMW_ERR_ARG, "mmw_carry from itself");
            expect(mmw_carry(nullptr, ha.s) == MMW_ERR_ARG && mmw_carry(hb.s, nullptr) == MMW_ERR_ARG, "mmw_carry null handles");
            expect(mmw_carry_map(hb.s, nullptr, nullptr, 0, nullptr, 0) == MMW_ERR_ARG, "mmw_carry_map null handle");
        }
    State small(4), large(9);
    Handle hs(small, MMW_F64, 2), hl(large, MMW_F64, 2);
    std::vector<int32_t> m(256, 0);
    if (hs.s && hl.s) expect(mmw_carry_map(hs.s, hl.s, m.data(), hs.sz[4], m.data(), hs.sz[8]) == MMW_ERR_ARG, "another K refused");
    std::printf(failures ? "host_carry_check: %d FAILED\n" : "host_carry_check: ok\n", failures);
    return failures ? 1 : 0;
}
