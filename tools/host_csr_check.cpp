// Developer tool (build container, no GPU): the host side of the device CSR entry point (mmw_csr_* with device -1, mmw_create_from_csr on
// it) driven through the C ABI from a program of its own, so that the shared validator (csr_check_row, pattern_csr_device.h: the very
// statements the kernels run), the host bounds and the hand-over to build_pattern can be run under the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-inline-asm -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/host_csr_check.cpp sig_sdp_mmw_amd/csrc/mmw_api.hip -o host_csr_check && ./host_csr_check
// Every array is a heap allocation of exactly the announced length, so a read past an array's end -- the thing the validation order
// exists to prevent (indptr before indices, column ranges before a column is an address) -- is reported by the sanitizer.
// A valid K = 6 state is accepted and compared with mmw_create's handle; then one field is spoiled at a time, including the kinds no
// GPU test may show a device (indptr[0], decreasing indptr, indptr[K] beyond the announced nnz, columns out of range, negative columns).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mmw_hip.h"

static int failures = 0;
static void expect(bool ok, const std::string& what) {
    if (!ok) { ++failures; std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what.c_str(), mmw_last_error()); }
}

struct State {
    int K = 6;
    std::vector<int32_t> Sp, Si, Qp, Qi;
    std::vector<double> Sx, Qx, h;
    State() {  // users 0-1 and 2-3 are association pairs; user 4 neither emits nor hears; gains elsewhere, own gain on the diagonal
        Sp.push_back(0); Qp.push_back(0);
        for (int a = 0; a < K; ++a) {
            for (int b = 0; b < K; ++b) {
                const bool gain = a != 4 && b != 4 && a != b && (a * 7 + b * 3) % 4 != 0;
                if (a == b || gain) { Si.push_back(b); Sx.push_back(a == b ? 3.0 : 0.25 + 0.1 * a + 0.01 * b); }
            }
            Sp.push_back((int32_t)Si.size());
            if (a < 4) { Qi.push_back(a ^ 1); Qx.push_back(1.0); }
            Qp.push_back((int32_t)Qi.size());
        }
        h.assign(K, 1.0);
    }
};
// upload (device -1) and create; returns the status of the first call that refused, message in mmw_last_error
static int build(const State& s, int Z, mmw_solver** out, int32_t bounds[2] = nullptr) {
    mmw_csr* c = nullptr;
    int rc = mmw_csr_upload(&c, -1, s.K, (int64_t)s.Si.size(), (int64_t)s.Qi.size(), s.Sp.data(), s.Si.empty() ? nullptr : s.Si.data(), s.Sx.empty() ? nullptr : s.Sx.data(),
                            s.Qp.data(), s.Qi.empty() ? nullptr : s.Qi.data(), s.Qx.empty() ? nullptr : s.Qx.data(), s.h.data());
    if (rc != MMW_OK) return rc;
    rc = mmw_create_from_csr(out, c, MMW_F64, Z, 2, 0.1, 3);
    if (bounds) {
        expect(mmw_csr_bounds(c, bounds) == MMW_OK, "bounds of a valid state");
    }
    mmw_csr_destroy(c);
    return rc;
}
static void refused(const State& s, int Z, const char* words) {
    mmw_solver* h = nullptr;
    const int rc = build(s, Z, &h);
    expect(rc == MMW_ERR_ARG && h == nullptr, std::string("refused: ") + words);
    expect(std::strstr(mmw_last_error(), words) != nullptr, std::string("message has: ") + words);
    if (h) mmw_destroy(h);
}

int main() {
    {  // the valid state: the handle is mmw_create's
        State s;
        mmw_solver *a = nullptr, *b = nullptr;
        int32_t bnd[2] = {0, 0};
        expect(build(s, 3, &b, bnd) == MMW_OK, "valid state accepted");
        expect(mmw_create(&a, -1, MMW_F64, s.K, 3, 2, 0.1, 3, s.Sp.data(), s.Si.data(), s.Sx.data(), s.Qp.data(), s.Qi.data(), s.Qx.data(), s.h.data()) == MMW_OK, "mmw_create");
        int64_t sa[10], sb[10];
        expect(mmw_sizes(a, sa) == MMW_OK && mmw_sizes(b, sb) == MMW_OK && std::memcmp(sa, sb, sizeof sa) == 0, "same sizes");
        std::vector<int32_t> la((size_t)sa[4]), lb((size_t)sb[4]);
        expect(mmw_read_i32(a, MMW_I_L_INDICES, la.data(), sa[4]) == MMW_OK && mmw_read_i32(b, MMW_I_L_INDICES, lb.data(), sb[4]) == MMW_OK && la == lb, "same l_indices");
        expect(bnd[0] == 2 && bnd[1] >= 3, "bounds of the valid state");
        mmw_destroy(a); mmw_destroy(b);
    }
    {  // K = 3 without Q: null index / data pointers where the length is 0
        State s;
        s.K = 3; s.Sp = {0, 1, 1, 1}; s.Si = {2}; s.Sx = {0.7}; s.Qp = {0, 0, 0, 0}; s.Qi.clear(); s.Qx.clear(); s.h.assign(3, 1.0);
        mmw_solver* h = nullptr;
        expect(build(s, 3, &h) == MMW_OK, "K = 3 without Q");
        if (h) mmw_destroy(h);
    }
    { State s; s.Sp[0] = 1; refused(s, 3, "indptr[0] must be 0"); }
    { State s; s.Qp[0] = -1; refused(s, 3, "indptr[0] must be 0"); }
    { State s; s.Sp[2] = s.Sp[1] - 1; refused(s, 3, "indptr must be non-decreasing"); }
    { State s; s.Sp[6] += 1000; refused(s, 3, "indptr[K] must equal"); }
    { State s; s.Qp[6] += 1; refused(s, 3, "indptr[K] must equal"); }
    { State s; s.Sp[3] = 1 << 30; refused(s, 3, "indptr must be non-decreasing"); }  // (a huge offset in the middle: the next one is smaller)
    { State s; s.Si[3] = 6; refused(s, 3, "S_gain column index out of range"); }
    { State s; s.Si[3] = -1; refused(s, 3, "S_gain column index out of range"); }
    { State s; s.Qi[1] = 1 << 20; refused(s, 3, "Q_asso column index out of range"); }
    { State s; std::swap(s.Si[0], s.Si[1]); refused(s, 3, "S_gain must be canonical CSR"); }
    { State s; s.Si[1] = s.Si[0]; refused(s, 3, "S_gain must be canonical CSR"); }
    { State s; s.Qx[0] = 0.0; refused(s, 3, "Q_asso must not store explicit zeros"); }
    { State s; s.Qi[0] = 0; refused(s, 3, "Q_asso must have an empty diagonal"); }
    { State s; s.Qi.erase(s.Qi.begin() + 1); s.Qx.pop_back(); for (int k = 2; k <= 6; ++k) --s.Qp[k]; refused(s, 3, "Q_asso must be symmetric"); }
    { State s; refused(s, 1, "Z must be >= 2"); }
    { State s; s.h[4] = 0.0; refused(s, 3, "norm_H has a zero entry"); }
    {
        State s;
        s.K = 1; s.Sp = {0, 1}; s.Si = {0}; s.Sx = {3.0}; s.Qp = {0, 0}; s.Qi.clear(); s.Qx.clear(); s.h.assign(1, 1.0);
        refused(s, 3, "K must be >= 2");
    }
    {  // what the entry points themselves refuse
        mmw_csr* c = nullptr;
        State s;
        expect(mmw_csr_upload(&c, -1, 0, 0, 0, s.Sp.data(), nullptr, nullptr, s.Qp.data(), nullptr, nullptr, s.h.data()) == MMW_ERR_ARG && !c, "K = 0 refused");
        expect(mmw_csr_upload(&c, -1, s.K, (int64_t)s.Si.size(), (int64_t)s.Qi.size(), s.Sp.data(), nullptr, s.Sx.data(), s.Qp.data(), s.Qi.data(), s.Qx.data(), s.h.data()) == MMW_ERR_ARG && !c,
               "null indices with a length refused");
        expect(mmw_csr_wrap(&c, -1, s.K, 0, 0, s.Sp.data(), nullptr, nullptr, s.Qp.data(), nullptr, nullptr, s.h.data()) == MMW_ERR_ARG && !c, "wrap with device -1 refused");
    }
    std::printf(failures ? "%d FAILURES\n" : "host_csr_check: ok\n", failures);
    return failures ? 1 : 0;
}
