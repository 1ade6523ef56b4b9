// State processing ON THE DEVICE from a CSR state that already lies there (mmw_create_from_csr, csr_device.h): everything build_pattern
// (pattern.h) derives from the seven arrays S_gain (indptr, indices, data), Q_asso (same) and h_max -- mmw._process_state and the
// prologue of mmw._run (sim_src/alg/mmw.py:26-60) for a general graph.
//
//   validation   k_csr_check, three launches that gate each other through a word each: the indptr arrays, then the column ranges,
//                then whatever uses a column as an address (order, stored zeros, diagonal and symmetry of Q).  The per-row checks are
//                csr_check_row, which the host path runs in a plain loop.  The first error is the lowest (class, row): an integer min.
//   rows of S    k_csrpat_count / k_csrpat_fill: row j without its diagonal and stored zeros (the rounding's lists), and of those the
//                entries (j, k) with (k, j) not in nz(Q) (the filtered row f; membership by binary search in Q's sorted row k).
//   S_T' = f^T   column counts by integer atomics, placement in arrival order, then k_csrpat_sort_rows ranks every row's (unique)
//                keys: the result does not depend on the arrival order.
//   L / X rows   k_csrpat_count_L / k_csrpat_fill_L: row a = {a} + S_T' row a + f row a + Q row a.  The three lists are sorted, so an
//                entry's place in the merged row is a sum of lower bounds; the one term that is not (entries of f that S_T' does not
//                hold already, below a column) is a running count the count pass leaves per entry of f.  Every entry is placed on its
//                own: rows of any length, no order between lanes, waves or workgroups.
//   edge lists   pair ids in triu-CSR order of Q from lower bounds in Q's rows; the upper gain edges by an ordered compaction of the
//                finished rows.
// Mirrors and the row statistics are pattern_device.h's kernels.  No float atomics, no grid barriers, no spin-waits.
#pragma once
#include "device_utils.h"
#include "runtime.h"

namespace mmw {

struct CsrView {  // the seven arrays, on the device or (device -1) on the host
    int K = 0;
    int nnzS = 0, nnzQ = 0;
    const int* Sp = nullptr; const int* Si = nullptr; const double* Sx = nullptr;
    const int* Qp = nullptr; const int* Qi = nullptr; const double* Qx = nullptr;
    const double* h = nullptr;
};

// ---- validation -----------------------------------------------------------------------------------------------------------------
enum CsrErrClass : int { CSR_E_PTR0 = 0, CSR_E_PTR_DEC, CSR_E_PTR_END, CSR_E_RANGE, CSR_E_ORDER, CSR_E_QZERO, CSR_E_QDIAG, CSR_E_QASYM };
constexpr unsigned long long CSR_OK = ~0ull;
constexpr int CSR_PHASES = 3;
__host__ __device__ inline unsigned long long csr_err_key(int cls, int row, int is_q) {
    return ((unsigned long long)cls << 33) | ((unsigned long long)(unsigned)row << 1) | (unsigned long long)is_q;
}
__host__ __device__ inline unsigned long long csr_err_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }
// first position in idx[lo, hi) whose value is >= c (the row is sorted)
__host__ __device__ inline int csr_lower(const int* idx, int lo, int hi, int c) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__host__ __device__ inline bool csr_has(const int* idx, int lo, int hi, int c) {
    const int w = csr_lower(idx, lo, hi, c);
    return w < hi && idx[w] == c;
}
// The checks of row k in one phase; the row's entries lane, lane + step, ... (host: 0, 1).  Phase 0 reads the indptr arrays only; phase 1
// (after 0 passed: every indptr value lies in [0, nnz]) the column ranges; phase 2 (after 1 passed) may use a column as a row number.
__host__ __device__ inline unsigned long long csr_check_row(const CsrView& V, int phase, int k, int lane, int step) {
    unsigned long long e = CSR_OK;
    if (phase == 0) {
        if (lane != 0) return e;
        if (k == 0 && V.Sp[0] != 0) e = csr_err_min(e, csr_err_key(CSR_E_PTR0, 0, 0));
        if (k == 0 && V.Qp[0] != 0) e = csr_err_min(e, csr_err_key(CSR_E_PTR0, 0, 1));
        if (V.Sp[k + 1] < V.Sp[k]) e = csr_err_min(e, csr_err_key(CSR_E_PTR_DEC, k, 0));
        if (V.Qp[k + 1] < V.Qp[k]) e = csr_err_min(e, csr_err_key(CSR_E_PTR_DEC, k, 1));
        if (k == V.K - 1 && V.Sp[V.K] != V.nnzS) e = csr_err_min(e, csr_err_key(CSR_E_PTR_END, k, 0));
        if (k == V.K - 1 && V.Qp[V.K] != V.nnzQ) e = csr_err_min(e, csr_err_key(CSR_E_PTR_END, k, 1));
        return e;
    }
    const int sb = V.Sp[k], se = V.Sp[k + 1], qb = V.Qp[k], qe = V.Qp[k + 1];
    if (phase == 1) {
        for (int i = sb + lane; i < se; i += step)
            if (V.Si[i] < 0 || V.Si[i] >= V.K) e = csr_err_min(e, csr_err_key(CSR_E_RANGE, k, 0));
        for (int i = qb + lane; i < qe; i += step)
            if (V.Qi[i] < 0 || V.Qi[i] >= V.K) e = csr_err_min(e, csr_err_key(CSR_E_RANGE, k, 1));
        return e;
    }
    for (int i = sb + lane; i < se; i += step)
        if (i > sb && V.Si[i] <= V.Si[i - 1]) e = csr_err_min(e, csr_err_key(CSR_E_ORDER, k, 0));
    for (int i = qb + lane; i < qe; i += step) {
        const int c = V.Qi[i];
        if (i > qb && c <= V.Qi[i - 1]) e = csr_err_min(e, csr_err_key(CSR_E_ORDER, k, 1));
        if (V.Qx[i] == 0.0) e = csr_err_min(e, csr_err_key(CSR_E_QZERO, k, 1));
        if (c == k) e = csr_err_min(e, csr_err_key(CSR_E_QDIAG, k, 1));
        if (!csr_has(V.Qi, V.Qp[c], V.Qp[c + 1], k)) e = csr_err_min(e, csr_err_key(CSR_E_QASYM, k, 1));
    }
    return e;
}
// build_pattern's words for each kind
inline std::string csr_err_text(unsigned long long key) {
    const int cls = (int)(key >> 33);
    const bool q = (key & 1ull) != 0;
    const std::string who = q ? "Q_asso" : "S_gain";
    switch (cls) {
        case CSR_E_PTR0: return "indptr[0] must be 0 (" + who + ")";
        case CSR_E_PTR_DEC: return "indptr must be non-decreasing (" + who + ")";
        case CSR_E_PTR_END: return "indptr[K] must equal the number of stored entries announced (" + who + ")";
        case CSR_E_RANGE: return who + " column index out of range";
        case CSR_E_ORDER: return who + " must be canonical CSR (sorted, no duplicates)";
        case CSR_E_QZERO: return "Q_asso must not store explicit zeros";
        case CSR_E_QDIAG: return "Q_asso must have an empty diagonal";
        default: return "Q_asso must be symmetric";
    }
}
__host__ __device__ inline bool csr_all_ok(const unsigned long long* err) { return err[0] == CSR_OK && err[1] == CSR_OK && err[2] == CSR_OK; }
// the three phases on the host (device -1)
inline void csr_check_host(const CsrView& V, unsigned long long err[CSR_PHASES]) {
    for (int p = 0; p < CSR_PHASES; ++p) err[p] = CSR_OK;
    for (int p = 0; p < CSR_PHASES; ++p) {
        for (int k = 0; k < V.K; ++k) err[p] = csr_err_min(err[p], csr_check_row(V, p, k, 0, 1));
        if (err[p] != CSR_OK) return;
    }
}
// err[p] = lowest key of phase p; a phase runs only if every phase before it (an earlier launch) passed
__global__ __launch_bounds__(BLOCK) void k_csr_check(CsrView V, int phase, unsigned long long* __restrict__ err) {
    for (int p = 0; p < phase; ++p)
        if (err[p] != CSR_OK) return;
    unsigned long long e = CSR_OK;
    if (phase == 0) {
        for (int k = blockIdx.x * BLOCK + threadIdx.x; k < V.K; k += gridDim.x * BLOCK) e = csr_err_min(e, csr_check_row(V, 0, k, 0, 1));
    } else {
        const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
        for (int k = blockIdx.x * WAVES_PER_BLOCK + wib; k < V.K; k += gridDim.x * WAVES_PER_BLOCK) e = csr_err_min(e, csr_check_row(V, phase, k, lane, WAVE));
    }
    if (e != CSR_OK) atomicMin(&err[phase], e);
}

// ---- the bisection's bounds (binary_search_relaxation.py:13-29): per row a, #{j != a : S[a,j] != 0} - #{those with S[j,a] != 0 too}, and
// per column the count of its stored non-zeros off the diagonal (integer atomics); the host adds the two and takes the maximum
__global__ __launch_bounds__(BLOCK) void k_csr_sym_count(CsrView V, const unsigned long long* __restrict__ err, int* __restrict__ row_only, int* __restrict__ col_cnt) {
    if (!csr_all_ok(err)) return;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int a = blockIdx.x * WAVES_PER_BLOCK + wib; a < V.K; a += gridDim.x * WAVES_PER_BLOCK) {
        int r = 0;
        for (int i = V.Sp[a] + lane; i < V.Sp[a + 1]; i += WAVE) {
            const int c = V.Si[i];
            if (c == a || V.Sx[i] == 0.0) continue;
            atomicAdd(&col_cnt[c], 1);
            const int w = csr_lower(V.Si, V.Sp[c], V.Sp[c + 1], a);
            const bool both = w < V.Sp[c + 1] && V.Si[w] == a && V.Sx[w] != 0.0;
            if (!both) ++r;
        }
        r = wave_sum(r);
        if (lane == 0) row_only[a] = r;
    }
}

// ---- rows of S: pass 1, the lengths {rounding row, filtered row f, triu(Q, 1) row} and the column counts of f (= row lengths of S_T')
__global__ __launch_bounds__(BLOCK) void k_csrpat_count(CsrView V, const unsigned long long* __restrict__ err, int* __restrict__ n_so, int* __restrict__ n_f,
                                                        int* __restrict__ st_cnt, int* __restrict__ n_qu) {
    if (!csr_all_ok(err)) return;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int j = blockIdx.x * WAVES_PER_BLOCK + wib; j < V.K; j += gridDim.x * WAVES_PER_BLOCK) {
        int cso = 0, cf = 0, cq = 0;
        for (int i = V.Sp[j] + lane; i < V.Sp[j + 1]; i += WAVE) {
            const int k = V.Si[i];
            if (k == j || V.Sx[i] == 0.0) continue;
            ++cso;
            if (csr_has(V.Qi, V.Qp[k], V.Qp[k + 1], j)) continue;  // (k, j) in nz(Q): mmw.py:29-30
            ++cf;
            atomicAdd(&st_cnt[k], 1);
        }
        for (int i = V.Qp[j] + lane; i < V.Qp[j + 1]; i += WAVE) cq += V.Qi[i] > j ? 1 : 0;
        cso = wave_sum(cso); cf = wave_sum(cf); cq = wave_sum(cq);
        if (lane == 0) { n_so[j] = cso; n_f[j] = cf; n_qu[j] = cq; }
    }
}
// pass 2: the rounding's lists and f in row order (ordered compaction by ballot); every entry of f also takes the next free place of
// its column's row of S_T' (unsorted copy: k_csrpat_sort_rows orders it)
__global__ __launch_bounds__(BLOCK) void k_csrpat_fill(CsrView V, const int* __restrict__ so_ptr, const int* __restrict__ f_ptr, const int* __restrict__ st_ptr,
                                                       int* __restrict__ cursor, int* __restrict__ so_idx, double* __restrict__ so_val, double* __restrict__ so_hmax,
                                                       int* __restrict__ f_idx, double* __restrict__ f_val, int* __restrict__ tmp_idx, double* __restrict__ tmp_val) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j = blockIdx.x * WAVES_PER_BLOCK + wib; j < V.K; j += gridDim.x * WAVES_PER_BLOCK) {
        int oso = so_ptr[j], of = f_ptr[j];
        const int se = V.Sp[j + 1];
        for (int i0 = V.Sp[j]; i0 < se; i0 += WAVE) {
            const int i = i0 + lane;
            const bool in = i < se;
            const int k = in ? V.Si[i] : j;
            const double v = in ? V.Sx[i] : 0.0;
            const bool so = in && k != j && v != 0.0;
            bool f = false;
            if (so) f = !csr_has(V.Qi, V.Qp[k], V.Qp[k + 1], j);
            const unsigned long long mso = __ballot(so), mf = __ballot(f);
            if (so) {
                const int e = oso + __popcll(mso & below);
                so_idx[e] = k;
                so_val[e] = v;
                so_hmax[e] = V.h[k];
            }
            if (f) {
                const int e = of + __popcll(mf & below);
                f_idx[e] = k;
                f_val[e] = v;
                const int t = st_ptr[k] + atomicAdd(&cursor[k], 1);
                tmp_idx[t] = j;
                tmp_val[t] = v;
            }
            oso += __popcll(mso); of += __popcll(mf);
        }
    }
}
// every row of S_T' in ascending column order: an entry's place is the number of smaller keys in its row (the keys are unique)
__global__ __launch_bounds__(BLOCK) void k_csrpat_sort_rows(int K, const int* __restrict__ st_ptr, const int* __restrict__ tmp_idx, const double* __restrict__ tmp_val,
                                                            int* __restrict__ st_idx, double* __restrict__ st_val) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int k = blockIdx.x * WAVES_PER_BLOCK + wib; k < K; k += gridDim.x * WAVES_PER_BLOCK) {
        const int b = st_ptr[k], n = st_ptr[k + 1] - b;
        for (int i = lane; i < n; i += WAVE) {
            const int key = tmp_idx[b + i];
            int r = 0;
            for (int t = 0; t < n; ++t) r += tmp_idx[b + t] < key ? 1 : 0;
            st_idx[b + r] = key;
            st_val[b + r] = tmp_val[b + i];
        }
    }
}
// ---- L / X rows: pass 1.  fx[i] = entries of f before i in its row that S_T' does not hold; n_fnew[a] their number in the whole row;
// n_l[a] the merged row's length, n_gu[a] its gain entries above the diagonal
__global__ __launch_bounds__(BLOCK) void k_csrpat_count_L(CsrView V, const int* __restrict__ st_ptr, const int* __restrict__ st_idx, const int* __restrict__ f_ptr,
                                                          const int* __restrict__ f_idx, int* __restrict__ fx, int* __restrict__ n_fnew, int* __restrict__ n_l,
                                                          int* __restrict__ n_gu) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int a = blockIdx.x * WAVES_PER_BLOCK + wib; a < V.K; a += gridDim.x * WAVES_PER_BLOCK) {
        const int sb = st_ptr[a], se = st_ptr[a + 1], fb = f_ptr[a], fe = f_ptr[a + 1];
        int run = 0, cg = 0;
        for (int i0 = fb; i0 < fe; i0 += WAVE) {
            const int i = i0 + lane;
            const bool in = i < fe;
            const int c = in ? f_idx[i] : 0;
            const bool nw = in && !csr_has(st_idx, sb, se, c);
            const unsigned long long m = __ballot(nw);
            if (in) fx[i] = run + __popcll(m & below);
            cg += __popcll(__ballot(nw && c > a));
            run += __popcll(m);
        }
        if (lane == 0) {
            n_fnew[a] = run;
            n_l[a] = 1 + (se - sb) + run + (V.Qp[a + 1] - V.Qp[a]);
            n_gu[a] = (se - csr_lower(st_idx, sb, se, a)) + cg;
        }
    }
}
template <typename T> struct CsrPatOut {
    const int* l_ptr; const int* st_ptr; const int* f_ptr; const int* qu_ptr;
    const int* st_idx; const double* st_val; const int* f_idx; const double* f_val; const int* fx; const int* n_fnew;
    int* l_idx; int* lrow; T* sab; T* sba; int* pid; int* diag_pos;
    int* asso_x; int* asso_y; int* asso_pos;
    int* internal;  // set when a gain value sits on an association pair (the host build's internal error)
};
// pass 2: every entry of the three lists, and the diagonal, goes to (entries of the merged row below its column)
template <typename T> __global__ __launch_bounds__(BLOCK) void k_csrpat_fill_L(CsrView V, CsrPatOut<T> O) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    for (int a = blockIdx.x * WAVES_PER_BLOCK + wib; a < V.K; a += gridDim.x * WAVES_PER_BLOCK) {
        const int sb = O.st_ptr[a], se = O.st_ptr[a + 1], fb = O.f_ptr[a], fe = O.f_ptr[a + 1], qb = V.Qp[a], qe = V.Qp[a + 1];
        const int base = O.l_ptr[a], nfn = O.n_fnew[a];
        auto fnew_below = [&](int w) { return w < fe ? O.fx[w] : nfn; };  // w: a lower bound in f's row
        for (int i = sb + lane; i < se; i += WAVE) {  // S_T'[a][c], with S_T'[c][a] when f holds c too
            const int c = O.st_idx[i];
            const int wf = csr_lower(O.f_idx, fb, fe, c);
            const bool both = wf < fe && O.f_idx[wf] == c;
            const int e = base + (i - sb) + fnew_below(wf) + (csr_lower(V.Qi, qb, qe, c) - qb) + (a < c ? 1 : 0);
            O.l_idx[e] = c; O.lrow[e] = a;
            O.sab[e] = (T)O.st_val[i];
            O.sba[e] = both ? (T)O.f_val[wf] : (T)0;
            O.pid[e] = -1;
        }
        for (int i = fb + lane; i < fe; i += WAVE) {  // S_T'[c][a] alone
            const int c = O.f_idx[i];
            const int ws = csr_lower(O.st_idx, sb, se, c);
            if (ws < se && O.st_idx[ws] == c) continue;
            const int e = base + (ws - sb) + O.fx[i] + (csr_lower(V.Qi, qb, qe, c) - qb) + (a < c ? 1 : 0);
            O.l_idx[e] = c; O.lrow[e] = a;
            O.sab[e] = (T)0;
            O.sba[e] = (T)O.f_val[i];
            O.pid[e] = -1;
        }
        const int q_above = csr_lower(V.Qi, qb, qe, a);  // row a of triu(Q, 1) starts here (Q has no diagonal)
        for (int i = qb + lane; i < qe; i += WAVE) {  // association pairs: id in triu-CSR order of Q (mmw.py:57)
            const int c = V.Qi[i];
            const int ws = csr_lower(O.st_idx, sb, se, c), wf = csr_lower(O.f_idx, fb, fe, c);
            if ((ws < se && O.st_idx[ws] == c) || (wf < fe && O.f_idx[wf] == c)) *O.internal = 1;
            const int e = base + (ws - sb) + fnew_below(wf) + (i - qb) + (a < c ? 1 : 0);
            int id;
            if (c > a) {
                id = O.qu_ptr[a] + (i - q_above);
                O.asso_x[id] = a; O.asso_y[id] = c; O.asso_pos[id] = e;
            } else {
                const int cb = V.Qp[c], ce = V.Qp[c + 1];
                id = O.qu_ptr[c] + (csr_lower(V.Qi, cb, ce, a) - csr_lower(V.Qi, cb, ce, c));
            }
            O.l_idx[e] = c; O.lrow[e] = a;
            O.sab[e] = (T)0; O.sba[e] = (T)0;
            O.pid[e] = id;
        }
        if (lane == 0) {
            const int e = base + (csr_lower(O.st_idx, sb, se, a) - sb) + fnew_below(csr_lower(O.f_idx, fb, fe, a)) + (q_above - qb);
            O.l_idx[e] = a; O.lrow[e] = a;
            O.sab[e] = (T)0; O.sba[e] = (T)0;
            O.pid[e] = -1;
            O.diag_pos[a] = e;
        }
    }
}
// the upper-triangular gain edges in CSR row-major order of the finished pattern
__global__ __launch_bounds__(BLOCK) void k_csrpat_gain_edges(int K, const int* __restrict__ l_ptr, const int* __restrict__ l_idx, const int* __restrict__ pid,
                                                             const int* __restrict__ gu_ptr, int* __restrict__ gain_x, int* __restrict__ gain_y) {
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int a = blockIdx.x * WAVES_PER_BLOCK + wib; a < K; a += gridDim.x * WAVES_PER_BLOCK) {
        int o = gu_ptr[a];
        const int le = l_ptr[a + 1];
        for (int e0 = l_ptr[a]; e0 < le; e0 += WAVE) {
            const int e = e0 + lane;
            const bool up = e < le && l_idx[e] > a && pid[e] < 0;
            const unsigned long long m = __ballot(up);
            if (up) {
                const int w = o + __popcll(m & below);
                gain_x[w] = a;
                gain_y[w] = l_idx[e];
            }
            o += __popcll(m);
        }
    }
}

}  // namespace mmw
