// State processing on the device for MANY instances given as CSR states that lie there (mmw_batch_create_from_csr), one workgroup per
// instance: pattern_csr_device.h restated for one workgroup and for the two arenas the batched solver reads (BatchDesc, kernels_batch.h),
// as kernels_batch_pattern.h restates pattern_device.h for a BatchEnv.  The per-instance table (BcsrItem: the seven pointers, the sizes
// and where the instance's work buffers lie) is the call's only input.
//
// The rules are pattern.h's: f = S without its diagonal, its stored zeros and the entries on association pairs ((k, j) in nz(Q), looked
// up in Q's sorted row k); S_T' = f^T with sorted rows; row a of L / X = {a} + S_T' row a + f row a + Q row a in ascending column order;
// pair ids in the triu-CSR order of Q; S_sum and the squared row sums over S_T' row k in ascending column order with separately rounded
// products and sums.
//
// k_batch_csr_count, phase by phase (a __syncthreads between them; every phase is a loop of one wave per row unless said):
//   check     csr_check_row's three phases, the lowest key of each by an integer minimum in LDS; a phase runs only when the ones before
//             passed, and an instance with a failed phase writes its three keys and NOTHING else: no column of it is used as an address.
//   rows of S lengths of the rounding row (so), of f and of triu(Q, 1) per row; the column counts of f (= row lengths of S_T') by integer
//             adds, whose order reaches nothing.  Four waves scan the four lists (benv_scan).
//   S_T'      f in row order (ordered compaction by ballot); every entry also takes the next free place of its column's row of S_T'
//             (integer add: arrival order), then every row is ranked by its (unique) keys: the result does not depend on the arrival.
//   L rows    per entry of f the count of earlier entries of its row that S_T' does not hold, per row the merged length and the gain
//             entries above the diagonal (k_csrpat_count_L); S_sum, the squared row sum and h_max by one thread per row.
// It leaves in the readback buffer the verdicts, l_indptr, the totals, the list lengths and the three vectors, and in the work buffers
// f, S_T', fx and the row pointers for the fill pass.
// k_batch_csr_fill: every entry of the three lists and the diagonal goes to (entries of the merged row below its column), a sum of
// lower bounds (k_csrpat_fill_L): rows of any length, no order between lanes or waves.  Then the rest of the instance's slices of the
// two arenas and the batch's own copy of the state (BatchPatItem), the so_* lists by an ordered compaction with so_hmax of every column.
//
// LDS: 3 keys and 8 partial totals (56 bytes); nothing is sized by K: the per-row and per-entry lists are global work buffers.  No float atomics; the integer adds above are counts and
// cursors whose arrival order no result keeps.  Nothing waits across workgroups, every address has one writer, every value depends on
// the instance's own arrays only: an instance is bitwise the same alone and among neighbours.
#pragma once
#include "kernels_batch_pattern.h"
#include "pattern_csr_device.h"

namespace mmw {

constexpr int BCSR_TOTALS = 5;    // ints per instance behind its l_indptr in the readback: nnzL, nnz(S_T'), E_gain, E_asso, nnz(so)
constexpr int BCSR_ROW_LISTS = 6;  // int work arrays of K + 1 entries: so_ptr, f_ptr, st_ptr, qu_ptr, cursor, n_fnew
constexpr int BCSR_ENT_LISTS = 4;  // int work arrays of nnz(S) entries: f_idx, tmp_idx, st_idx, fx
constexpr int BCSR_ENT_VALS = 3;   // fp64 work arrays of nnz(S) entries: f_val, tmp_val, st_val

struct BcsrItem {
    CsrView V;
    int64_t o_k;   // users of the instances before this one
    int64_t o_wi;  // its int work arrays
    int64_t o_wf;  // its fp64 work arrays
};
static_assert(sizeof(BcsrItem) % sizeof(double) == 0, "the table is uploaded as doubles");

// The readback: per instance the three validation keys (uint64), then S_sum, the squared row sums and h_max of all users side by
// side, then as int32 per instance l_indptr[K + 1] and the totals.
__host__ __device__ inline int64_t bcsr_rb_doubles(int64_t Ktot, int64_t B) { return CSR_PHASES * B + 3 * Ktot + (Ktot + (BCSR_TOTALS + 1) * B + 1) / 2; }
__host__ __device__ inline int64_t bcsr_rb_vec(int64_t B) { return CSR_PHASES * B; }
__host__ __device__ inline int64_t bcsr_rb_int0(int64_t Ktot, int64_t B) { return CSR_PHASES * B + 3 * Ktot; }  // in doubles
__host__ __device__ inline int64_t bcsr_rb_int(int64_t o_k, int64_t b) { return o_k + (BCSR_TOTALS + 1) * b; }
inline int64_t bcsr_wi_ints(int64_t K, int64_t ns) { return a32(BCSR_ROW_LISTS * (K + 1) + BCSR_ENT_LISTS * ns); }
inline int64_t bcsr_wf_doubles(int64_t ns) { return a32(BCSR_ENT_VALS * ns); }

struct BcsrWork {  // an instance's work arrays
    int *so_ptr, *f_ptr, *st_ptr, *qu_ptr, *cursor, *n_fnew, *f_idx, *tmp_idx, *st_idx, *fx;
    double *f_val, *tmp_val, *st_val;
};
__device__ __forceinline__ BcsrWork bcsr_work(const BcsrItem& t, int* wi, double* wf) {
    const int64_t K1 = (int64_t)t.V.K + 1, ns = t.V.nnzS;
    BcsrWork w;
    int* p = wi + t.o_wi;
    w.so_ptr = p; w.f_ptr = p + K1; w.st_ptr = p + 2 * K1; w.qu_ptr = p + 3 * K1; w.cursor = p + 4 * K1; w.n_fnew = p + 5 * K1;
    p += BCSR_ROW_LISTS * K1;
    w.f_idx = p; w.tmp_idx = p + ns; w.st_idx = p + 2 * ns; w.fx = p + 3 * ns;
    double* q = wf + t.o_wf;
    w.f_val = q; w.tmp_val = q + ns; w.st_val = q + 2 * ns;
    return w;
}
// S_sum and the squared row sum of row k of S_T' (mmw.py:34,37-39 as pattern.h evaluates them): the stored entries in ascending
// column order, products and sums rounded separately
__device__ __forceinline__ void bcsr_rowstats(const double* st_val, int b, int e, double& s_out, double& q_out) {
#pragma clang fp contract(off)  // (a fused multiply-add would differ from the host's last bit)
    double s = 0.0, q = 0.0;
    for (int i = b; i < e; ++i) {
        const double v = st_val[i];
        const double vv = v * v;
        s = s + v;
        q = q + vv;
    }
    s_out = s;
    q_out = q;
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_csr_count(const BcsrItem* __restrict__ items, int64_t Ktot, double* rb, int* wi, double* wf) {
    const int B = (int)gridDim.x, b = (int)blockIdx.x;
    const BcsrItem t = items[b];
    const CsrView V = t.V;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = V.K;
    const unsigned long long below = (1ull << lane) - 1ull;
    __shared__ unsigned long long s_err[CSR_PHASES];
    __shared__ int s_tot[BATCH_WAVES];  // per wave: upper gain edges
    // ---- validation: nothing below uses a column as an address unless all three phases passed
    if (tid < CSR_PHASES) s_err[tid] = CSR_OK;
    __syncthreads();
    bool bad = false;
    for (int p = 0; p < CSR_PHASES && !bad; ++p) {
        unsigned long long e = CSR_OK;
        if (p == 0) {
            for (int k = tid; k < K; k += BATCH_THREADS) e = csr_err_min(e, csr_check_row(V, 0, k, 0, 1));
        } else {
            for (int k = wv; k < K; k += BATCH_WAVES) e = csr_err_min(e, csr_check_row(V, p, k, lane, WAVE));
        }
        if (e != CSR_OK) atomicMin(&s_err[p], e);
        __syncthreads();
        bad = s_err[p] != CSR_OK;  // (the same for every thread)
    }
    if (tid < CSR_PHASES) reinterpret_cast<unsigned long long*>(rb)[(int64_t)CSR_PHASES * b + tid] = s_err[tid];
    if (bad) return;
    const BcsrWork w = bcsr_work(t, wi, wf);
    double* vec = rb + bcsr_rb_vec(B);
    int* l_ptr = reinterpret_cast<int*>(rb + bcsr_rb_int0(Ktot, B)) + bcsr_rb_int(t.o_k, b);
    // ---- rows of S: the lengths, and the column counts of f
    for (int k = tid; k <= K; k += BATCH_THREADS) { w.st_ptr[k] = 0; w.cursor[k] = 0; }
    __syncthreads();
    for (int j = wv; j < K; j += BATCH_WAVES) {
        int cso = 0, cf = 0, cq = 0;
        for (int i = V.Sp[j] + lane; i < V.Sp[j + 1]; i += WAVE) {
            const int k = V.Si[i];
            if (k == j || V.Sx[i] == 0.0) continue;
            ++cso;
            if (csr_has(V.Qi, V.Qp[k], V.Qp[k + 1], j)) continue;  // (k, j) in nz(Q): mmw.py:29-30
            ++cf;
            atomicAdd(&w.st_ptr[k], 1);
        }
        for (int i = V.Qp[j] + lane; i < V.Qp[j + 1]; i += WAVE) cq += V.Qi[i] > j ? 1 : 0;
        cso = wave_sum(cso); cf = wave_sum(cf); cq = wave_sum(cq);
        if (lane == 0) { w.so_ptr[j] = cso; w.f_ptr[j] = cf; w.qu_ptr[j] = cq; }
    }
    __syncthreads();
    if (wv == 0) benv_scan(w.so_ptr, K);
    if (wv == 1) benv_scan(w.f_ptr, K);
    if (wv == 2) benv_scan(w.st_ptr, K);
    if (wv == 3) benv_scan(w.qu_ptr, K);
    __syncthreads();
    // ---- f in row order; every entry also takes the next free place of its column's row of S_T'
    for (int j = wv; j < K; j += BATCH_WAVES) {
        int of = w.f_ptr[j];
        const int se = V.Sp[j + 1];
        for (int i0 = V.Sp[j]; i0 < se; i0 += WAVE) {
            const int i = i0 + lane;
            const bool in = i < se;
            const int k = in ? V.Si[i] : j;
            const double v = in ? V.Sx[i] : 0.0;
            bool f = in && k != j && v != 0.0;
            if (f) f = !csr_has(V.Qi, V.Qp[k], V.Qp[k + 1], j);
            const unsigned long long mf = __ballot(f);
            if (f) {
                const int e = of + __popcll(mf & below);
                w.f_idx[e] = k;
                w.f_val[e] = v;
                const int d = w.st_ptr[k] + atomicAdd(&w.cursor[k], 1);
                w.tmp_idx[d] = j;
                w.tmp_val[d] = v;
            }
            of += __popcll(mf);
        }
    }
    __syncthreads();
    // ---- every row of S_T' in ascending column order: an entry's place is the number of smaller keys in its row
    for (int k = wv; k < K; k += BATCH_WAVES) {
        const int o = w.st_ptr[k], n = w.st_ptr[k + 1] - o;
        for (int i = lane; i < n; i += WAVE) {
            const int key = w.tmp_idx[o + i];
            int r = 0;
            for (int u = 0; u < n; ++u) r += w.tmp_idx[o + u] < key ? 1 : 0;
            w.st_idx[o + r] = key;
            w.st_val[o + r] = w.tmp_val[o + i];
        }
    }
    __syncthreads();
    // ---- the row statistics, and the lengths of the merged rows
    for (int k = tid; k < K; k += BATCH_THREADS) {
        double s, q;
        bcsr_rowstats(w.st_val, w.st_ptr[k], w.st_ptr[k + 1], s, q);
        vec[t.o_k + k] = s;
        vec[Ktot + t.o_k + k] = q;
        vec[2 * Ktot + t.o_k + k] = V.h[k];
    }
    int cG = 0;
    for (int a = wv; a < K; a += BATCH_WAVES) {
        const int sb = w.st_ptr[a], se = w.st_ptr[a + 1], fb = w.f_ptr[a], fe = w.f_ptr[a + 1];
        int run = 0;
        for (int i0 = fb; i0 < fe; i0 += WAVE) {
            const int i = i0 + lane;
            const bool in = i < fe;
            const int c = in ? w.f_idx[i] : 0;
            const bool nw = in && !csr_has(w.st_idx, sb, se, c);
            const unsigned long long m = __ballot(nw);
            if (in) w.fx[i] = run + __popcll(m & below);
            cG += __popcll(__ballot(nw && c > a));
            run += __popcll(m);
        }
        if (lane == 0) {
            w.n_fnew[a] = run;
            l_ptr[a] = 1 + (se - sb) + run + (V.Qp[a + 1] - V.Qp[a]);
        }
        cG += se - csr_lower(w.st_idx, sb, se, a);  // S_T' holds no diagonal: its entries above a
    }
    if (lane == 0) s_tot[wv] = cG;
    __syncthreads();
    if (wv == 0) benv_scan(l_ptr, K);
    __syncthreads();
    if (tid == 0) {
        int* tot = l_ptr + K + 1;
        tot[0] = l_ptr[K];
        tot[1] = w.st_ptr[K];
        tot[2] = 0;
        for (int u = 0; u < BATCH_WAVES; ++u) tot[2] += s_tot[u];
        tot[3] = w.qu_ptr[K];
        tot[4] = w.so_ptr[K];
    }
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_csr_fill(const BcsrItem* __restrict__ items, const BatchDesc* __restrict__ descs,
                                                                  const BatchPatItem* __restrict__ pitems, int64_t Ktot, const double* __restrict__ rb,
                                                                  int* wi, double* wf, const double* __restrict__ invn, const double* __restrict__ cH,
                                                                  int* __restrict__ ia, double* __restrict__ fa, int* __restrict__ si,
                                                                  double* __restrict__ sf) {
    const int B = (int)gridDim.x, b = (int)blockIdx.x;
    const BcsrItem t = items[b];
    const CsrView V = t.V;
    const BatchDesc& d = descs[b];
    const BatchPatItem pt = pitems[b];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = V.K;
    const int64_t nnz = d.nnzL;
    const unsigned long long below = (1ull << lane) - 1ull;
    const BcsrWork w = bcsr_work(t, wi, wf);
    const double* vec = rb + bcsr_rb_vec(B);
    const int* l_ptr = reinterpret_cast<const int*>(rb + bcsr_rb_int0(Ktot, B)) + bcsr_rb_int(t.o_k, b);
    int* col = ia + d.o_col;
    int* lrow = ia + d.o_lrow;
    int* pid = ia + d.o_pid;
    int* diag = ia + d.o_diag;
    int* apos = ia + d.o_apos;
    double* sab = fa + d.o_sab;
    double* sba = sab + nnz;
    int* so_idx = si + pt.c_soidx;
    double* so_val = sf + pt.v_soval;
    double* so_hmax = sf + pt.v_sohmax;
    for (int a = wv; a < K; a += BATCH_WAVES) {
        const int sb = w.st_ptr[a], se = w.st_ptr[a + 1], fb = w.f_ptr[a], fe = w.f_ptr[a + 1], qb = V.Qp[a], qe = V.Qp[a + 1];
        const int base = l_ptr[a], nfn = w.n_fnew[a];
        auto fnew_below = [&](int x) { return x < fe ? w.fx[x] : nfn; };  // x: a lower bound in f's row
        for (int i = sb + lane; i < se; i += WAVE) {  // S_T'[a][c], with S_T'[c][a] when f holds c too
            const int c = w.st_idx[i];
            const int xf = csr_lower(w.f_idx, fb, fe, c);
            const bool both = xf < fe && w.f_idx[xf] == c;
            const int e = base + (i - sb) + fnew_below(xf) + (csr_lower(V.Qi, qb, qe, c) - qb) + (a < c ? 1 : 0);
            col[e] = c; lrow[e] = a;
            sab[e] = w.st_val[i];
            sba[e] = both ? w.f_val[xf] : 0.0;
            pid[e] = -1;
        }
        for (int i = fb + lane; i < fe; i += WAVE) {  // S_T'[c][a] alone
            const int c = w.f_idx[i];
            const int xs = csr_lower(w.st_idx, sb, se, c);
            if (xs < se && w.st_idx[xs] == c) continue;
            const int e = base + (xs - sb) + w.fx[i] + (csr_lower(V.Qi, qb, qe, c) - qb) + (a < c ? 1 : 0);
            col[e] = c; lrow[e] = a;
            sab[e] = 0.0;
            sba[e] = w.f_val[i];
            pid[e] = -1;
        }
        const int q_above = csr_lower(V.Qi, qb, qe, a);  // row a of triu(Q, 1) starts here (Q has no diagonal)
        for (int i = qb + lane; i < qe; i += WAVE) {  // association pairs: id in triu-CSR order of Q (mmw.py:57)
            const int c = V.Qi[i];
            const int xs = csr_lower(w.st_idx, sb, se, c), xf = csr_lower(w.f_idx, fb, fe, c);
            const int e = base + (xs - sb) + fnew_below(xf) + (i - qb) + (a < c ? 1 : 0);
            int id;
            if (c > a) {
                id = w.qu_ptr[a] + (i - q_above);
                apos[id] = e;
            } else {
                const int cb = V.Qp[c], ce = V.Qp[c + 1];
                id = w.qu_ptr[c] + (csr_lower(V.Qi, cb, ce, a) - csr_lower(V.Qi, cb, ce, c));
            }
            col[e] = c; lrow[e] = a;
            sab[e] = 0.0; sba[e] = 0.0;
            pid[e] = id;
        }
        if (lane == 0) {
            const int e = base + (csr_lower(w.st_idx, sb, se, a) - sb) + fnew_below(csr_lower(w.f_idx, fb, fe, a)) + (q_above - qb);
            col[e] = a; lrow[e] = a;
            sab[e] = 0.0; sba[e] = 0.0;
            pid[e] = -1;
            diag[a] = e;
        }
        // the rounding's lists: row a of S without its diagonal and stored zeros, h_max of every stored column beside it
        int oso = w.so_ptr[a];
        const int ze = V.Sp[a + 1];
        for (int i0 = V.Sp[a]; i0 < ze; i0 += WAVE) {
            const int i = i0 + lane;
            const bool in = i < ze;
            const int k = in ? V.Si[i] : a;
            const double v = in ? V.Sx[i] : 0.0;
            const bool so = in && k != a && v != 0.0;
            const unsigned long long m = __ballot(so);
            if (so) {
                const int e = oso + __popcll(m & below);
                so_idx[e] = k;
                so_val[e] = v;
                so_hmax[e] = V.h[k];
            }
            oso += __popcll(m);
        }
    }
    bpat_copy(ia + d.o_indptr, l_ptr, (int64_t)K + 1);
    bpat_copy(fa + d.o_hmax, vec + 2 * Ktot + t.o_k, K);
    bpat_copy(fa + d.o_ssum, vec + t.o_k, K);
    bpat_copy(fa + d.o_invn, invn + pt.o_scal, K);
    bpat_copy(fa + d.o_cH, cH + pt.o_scal, K);
    // the batch's own copy of the state: no mmw_csr is referenced once the call returns
    bpat_copy(si + pt.c_sptr, V.Sp, (int64_t)K + 1);
    bpat_copy(si + pt.c_soptr, w.so_ptr, (int64_t)K + 1);
    bpat_copy(si + pt.c_qptr, V.Qp, (int64_t)K + 1);
    bpat_copy(si + pt.c_sidx, V.Si, V.nnzS);
    bpat_copy(si + pt.c_qidx, V.Qi, V.nnzQ);
    bpat_copy(sf + pt.v_hmax, V.h, K);
    bpat_copy(sf + pt.v_sval, V.Sx, V.nnzS);
    bpat_copy(sf + pt.v_qval, V.Qx, V.nnzQ);
}

}  // namespace mmw
