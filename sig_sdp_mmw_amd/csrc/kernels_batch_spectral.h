// The spectral baseline of a batched sweep on the device (mmw_batch_factor_spectral): spectral_sdp_solver.run_with_state
// (sim_src/alg/sdp_solver.py:165-185) -- the Laplacian of S_gain + S_gain^T without its diagonal, its Z eigenvectors of largest
// eigenvalue, the rows of that K x Z block normalised -- as the resident factor of every taking instance.
//
// The decomposition is the dense one-sided Jacobi the Xbar factor runs (epi_jacobi / k_batch_factor_round, unchanged): L is symmetric
// and positive semidefinite, so once its rows g_j are mutually orthogonal they are lambda_j v_j^T, the row norms are the eigenvalues
// and g_j / ||g_j|| is the eigenvector.  What this file adds is the head in front of the Jacobi and the tail behind it, both called
// from k_batch_factor and from k_batch_factor_head / _tail under FactorDesc::kind == 1 (a workgroup-uniform branch), so the single
// launch and the split chain run the same statements.
//
//   spectral_head   L = D - W, dense, in the instance's K x K work matrix from the state's rounding lists (S_gain without its diagonal):
//                   every stored entry scattered to its own cell; one thread per unordered pair {i, j} forms W_ij = S_ij + S_ji and
//                   writes -W_ij to both mirrors, so L is exactly symmetric; one wave per row sums the degree D_ii = sum_j W_ij, per-lane
//                   sums in ascending column order and the fixed-order wave reduction.  No atomics, no two threads add into one address.
//   spectral_tail   V[:, j] = g_row / ||g_row|| for the Z rows of largest norm, columns in ascending eigenvalue (eigsh's order), a row
//                   of norm 0 gives a zero column; then one wave per user divides that user's row of the K x Z block by its norm
//                   (sdp_solver.py:182), summed in the same fixed order.  A user whose row is exactly zero -- an isolated user is one:
//                   row and column of L are zero and no rotation touches them -- keeps a zero row, where the reference divides by zero.
//
// The eigenvector of eigenvalue 0 (the constant vector of a connected component) is the one the row norms cannot carry: its row ends
// as rounding noise, or as an exact zero.  It ranks last, so it enters the block only at Z = K.
#pragma once
#include "kernels_batch.h"

namespace mmw {

// L = D - W of the state's lists (soptr / soidx / sodata: row k = the stored S_gain[k, :] without the diagonal) into A (K x K, row-major).
// Ends with a workgroup barrier: A is final for every thread.
__device__ __forceinline__ void spectral_head(int K, const int* __restrict__ soptr, const int* __restrict__ soidx,
                                              const double* __restrict__ sodata, double* A) {
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
    const size_t KK = (size_t)K * K;
    for (size_t i = tid; i < KK; i += NT) A[i] = 0.0;
    __syncthreads();
    for (int row = wv; row < K; row += nw) {  // one wave per row of S: every stored entry has a cell of its own
        const int b = soptr[row], e = soptr[row + 1];
        for (int p = b + lane; p < e; p += WAVE) {
            const int c = soidx[p];
            if (c != row && (unsigned)c < (unsigned)K) A[(size_t)row * K + c] = sodata[p];
        }
    }
    __syncthreads();
    for (size_t idx = tid; idx < KK; idx += NT) {  // one thread per unordered pair: both mirrors from one sum
        const int i = (int)(idx / K), j = (int)(idx % K);
        if (i >= j) continue;
        const double w = A[idx] + A[(size_t)j * K + i];
        A[idx] = -w;
        A[(size_t)j * K + i] = -w;
    }
    __syncthreads();
    for (int row = wv; row < K; row += nw) {  // the degree: the diagonal cell is still 0 and takes no part in its own sum
        double s = 0.0;
        for (int c = lane; c < K; c += WAVE) s += A[(size_t)row * K + c];
        s = wave_sum(s);
        if (lane == 0) A[(size_t)row * K + row] = -s;
    }
    __syncthreads();
}

// The row-normalised eigenvector block fac[K, Z] from the orthogonal rows of A, their norms nrm[K] and ord[K] (rows by descending
// norm).  A workgroup barrier separates the columns from the pass over the rows; rown[K] keeps every user's row norm as it was
// before the division (MMW_F_FACTOR_ROWNORM: which users' rows are large enough to be trusted).
__device__ __forceinline__ void spectral_tail(int K, int Z, const double* A, const double* __restrict__ nrm, const int* __restrict__ ord,
                                              double* fac, double* __restrict__ rown) {
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & 63, wv = tid >> 6, nw = NT >> 6;
    const size_t KZ = (size_t)K * Z;
    for (size_t idx = tid; idx < KZ; idx += NT) {
        const int i = (int)(idx / Z), j = (int)(idx % Z);
        const int row = ord[Z - 1 - j];
        const double nv = nrm[row];
        fac[idx] = nv > 0.0 ? A[(size_t)row * K + i] / nv : 0.0;
    }
    __syncthreads();
    for (int k = wv; k < K; k += nw) {
        double* v = fac + (size_t)k * Z;
        double s = 0.0;
        for (int c = lane; c < Z; c += WAVE) s += v[c] * v[c];
        s = wave_sum(s);
        const double n = sqrt(s);
        if (lane == 0) rown[k] = n;
        if (n > 0.0)  // (wave-uniform) an exactly zero row stays zero
            for (int c = lane; c < Z; c += WAVE) v[c] /= n;
    }
}

}  // namespace mmw
