// The device tables of a handle's two locality blockings (blocking.h): host build threads, upload, kernel argument structs (the iterate's buffers are the core's, solver_core.h).
#pragma once
#include <queue>
#include <thread>

#include "blocking.h"
#include "expm_engine.h"
#include "kernels_loop.h"
#include "pattern.h"
#include "runtime.h"

namespace mmw {

template <typename T> BlockingLimits blocking_limits() { return BlockingLimits{blk_max_entries<T>(), (int)sizeof(BlkMeta<T>)}; }

template <typename T> struct BlockTables {
    HostBlocking HB;
    DevBuf<int> b_rowptr, b_order, b_unptr, b_uncols, b_bptr, b_bpos, b_bepos;
    DevBuf<unsigned short> b_lidx, b_selfli, b_sdla, b_sdlb;
    DevBuf<int> b_sdptr, b_sdepos, b_desc, b_unfixed;
    bool sddmm_blk = false;
    DevBuf<int> b_sd2ptr, b_sd2epos, b_sd2items;
    int sd2_nitems = 0;
    DevBuf<unsigned> b_sd2ab;
    bool sddmm_blk2 = false;  // half-tile SDDMM (k_sddmm_blk2)
    DevBuf<T> lval_blk;       // L in the LDS-staged SpMM's traversal order
    DevBuf<int> b_kbase, b_fpos, b_mdesc, b_munfixed, b_morder;  // matrix-core SpMM: its row blocks, CSR entry -> fragment image position
    DevBuf<unsigned> afrag;          // the matrix as bf16 hi << 16 | lo words in MFMA fragment order
    DevBuf<unsigned short> afrag16;  // the matrix as ONE fp16 half, for the first-order product while 2 * 2^-12 absn <= tol (holes zero; an image of its own)
    size_t afrag_n = 0;
    DevBuf<int> b_tbase, b_tptr;  // matrix-core SDDMM: pattern entries by 32 x 32 output tile
    DevBuf<unsigned short> b_trc, b_tmask;
    DevBuf<int> b_e2w, b_xasso;  // X in the matrix-core SDDMM's tile order: b_e2w maps a CSR entry to its slot, b_xasso an association pair
    size_t n_xs = 0;             // slots: undirected edges + K
    bool sddmm_mfma = false;
    // The host side of both blockings: one RCM order, then the two block builders on two threads (they fill disjoint parts of HB).
    // Reads only the pattern's structure, so init() starts it while build_pattern is still making the mirrors and edge lists.
    std::thread build_thread;
    bool blk_want_mf = false;
    void join() { if (build_thread.joinable()) build_thread.join(); }
    // whether the matrix-core blocking is wanted depends on the block's padded width only
    void want_mfma(int K, int D, const Switches& sw) {
        BlockLayout lay0;
        std::string lerr;
        blk_want_mf = sizeof(T) == 4 && !sw.no_mfma && make_layout(D, V16<T>::N, lay0, lerr) == MMW_OK && (double)K * lay0.Dpad * 4.0 < 4.0e9;
    }
    void host_blockings(const HostPattern& H, const Switches& sw) {
        const int Kp = H.K;
        bool rows_ok = true;
        for (int k = 0; k < Kp && rows_ok; ++k) rows_ok = H.l_indptr[k + 1] - H.l_indptr[k] <= BLK_UNION;
        if (rows_ok && HB.rcm_cache.size() != (size_t)Kp) HB.rcm_cache = rcm_order(Kp, H.l_indptr, H.l_indices);  // (a handle made from the generator brings a spatial order)
        std::thread mf_thread;
        if (blk_want_mf && rows_ok) mf_thread = std::thread([&]() { build_mfma_blocking(HB, Kp, H.l_indptr, H.l_indices, std::min(64, std::max(1, sw.mf_rows)), sw.mf_union_cap); });
        build_blocking(HB, Kp, H.l_indptr, H.l_indices, blocking_limits<T>());
        if (mf_thread.joinable()) mf_thread.join();
    }
    // Entry tables of the LDS-staged SDDMM kernels: built and uploaded on first need (a handle whose SDDMM runs on the matrix
    // cores never asks; blocking.h, build_sd_tables)
    bool sd_up = false;
    int ensure_sd(hipStream_t st, const HostPattern& H, int K, int Dpad, bool full_tile) {
        if (sd_up || !HB.usable) return MMW_OK;
        sd_up = true;
        build_sd_tables(HB, K, H.l_indptr, H.l_indices);
        // the block records carry every block's first slot of the half-tile SDDMM: refreshed in place (the kernels' argument
        // structs hold this buffer's address)
        if (b_desc.n != HB.desc.size()) return fail(MMW_ERR_STATE, "internal: block records changed size");
        MMW_HIP(hipMemcpyAsync(b_desc.p, HB.desc.data(), HB.desc.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (HB.sd_max <= SD_ROUNDS * BLK_THREADS) {
            MMW_TRY(b_sdptr.upload(HB.sd_ptr, st)); MMW_TRY(b_sdla.upload(HB.sd_la, st)); MMW_TRY(b_sdlb.upload(HB.sd_lb, st));
            MMW_TRY(b_sdepos.upload(HB.sd_epos, st));
            const size_t shb = (size_t)BLK_UNION_ROWS * BLK_TILE_BYTES;
            MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sddmm_blk<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shb));
            sddmm_blk = true;
        }
        if ((double)K * Dpad * sizeof(T) < 4.0e9 && !full_tile) {
            MMW_TRY(b_sd2ptr.upload(HB.sd2_ptr, st)); MMW_TRY(b_sd2ab.upload(HB.sd2_ab, st)); MMW_TRY(b_sd2epos.upload(HB.sd2_epos, st));
            {   // Work items.  A workgroup is a latency chain whose length is its number of rounds, and the launch lasts as long
                // as its longest workgroup; the resident slots the row blocks leave free are used to cut the longest items in two
                // (each half stages the union again).
                const int cus = device_cus();
                const int per_cu = std::max(1, std::min(2048 / SD2_THREADS, 163840 / std::max(1, HB.un8_max * B2_ROW_BYTES + 128)));
                const size_t slots = (size_t)per_cu * (size_t)cus;
                struct It { int rb, k0, k1; };
                auto len = [](const It& a) { return a.k1 - a.k0; };
                auto less = [&](const It& a, const It& b) { return len(a) != len(b) ? len(a) < len(b) : a.rb > b.rb; };
                std::priority_queue<It, std::vector<It>, decltype(less)> pq(less);
                for (int b = 0; b < HB.nb(); ++b) pq.push({b, 0, (HB.sd2_ptr[b + 1] - HB.sd2_ptr[b]) / SD2_THREADS});
                while ((pq.size() < slots && len(pq.top()) >= 2) || len(pq.top()) > sd2_rounds<T>()) {
                    const It t = pq.top();
                    pq.pop();
                    const int mid = t.k0 + (len(t) + 1) / 2;
                    pq.push({t.rb, t.k0, mid});
                    pq.push({t.rb, mid, t.k1});
                }
                std::vector<int32_t> items;
                while (!pq.empty()) {  // longest first
                    items.push_back(pq.top().rb); items.push_back(pq.top().k0); items.push_back(pq.top().k1);
                    pq.pop();
                }
                sd2_nitems = (int)(items.size() / 3);
                MMW_TRY(b_sd2items.upload(items, st));
            }
            MMW_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sddmm_blk2<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        std::max(HB.un8_max * B2_ROW_BYTES, 65536)));
            sddmm_blk2 = true;
        }
        MMW_HIP(hipStreamSynchronize(st));  // the uploads read host vectors
        return MMW_OK;
    }
    // The tables of a usable blocking, uploaded once the host threads are done.  `d_apos`: the pattern's association pairs on the device.
    int upload(hipStream_t st, const HostPattern& H, int K, const Switches& sw, const int* d_apos) {
        MMW_TRY(b_rowptr.upload(HB.blk_rowptr, st)); MMW_TRY(b_order.upload(HB.order, st)); MMW_TRY(b_unptr.upload(HB.un_ptr, st));
        MMW_TRY(b_uncols.upload(HB.un_cols, st)); MMW_TRY(b_bptr.upload(HB.bptr, st)); MMW_TRY(b_bpos.upload(HB.bpos, st));
        MMW_TRY(b_bepos.upload(HB.bepos, st)); MMW_TRY(b_lidx.upload(HB.lidx, st)); MMW_TRY(b_selfli.upload(HB.self_li, st)); MMW_TRY(b_desc.upload(HB.desc, st)); MMW_TRY(b_unfixed.upload(HB.un_fixed, st));
        MMW_TRY(lval_blk.alloc((size_t)HB.nent));
        if (sizeof(T) != 4 || !HB.fits_mfma) return MMW_OK;
        MMW_TRY(b_kbase.upload(HB.kbase, st));
        MMW_TRY(b_fpos.upload(HB.fpos, st));
        MMW_TRY(b_mdesc.upload(HB.m_desc, st));
        MMW_TRY(b_munfixed.upload(HB.m_unfixed, st));
        MMW_TRY(b_morder.upload(HB.m_order, st));
        afrag_n = (size_t)HB.kbase[HB.nbm()] * HB.mfma_mt * 512;
        MMW_TRY(afrag.alloc(afrag_n));
        MMW_HIP(hipMemsetAsync(afrag.p, 0, afrag_n * sizeof(unsigned), st));
        MMW_TRY(afrag16.alloc(afrag_n));
        MMW_HIP(hipMemsetAsync(afrag16.p, 0, afrag_n * sizeof(unsigned short), st));
        if (sw.no_mfma_sddmm) return MMW_OK;
        MMW_TRY(b_tbase.upload(HB.m_tbase, st)); MMW_TRY(b_tptr.upload(HB.m_tptr, st)); MMW_TRY(b_trc.upload(HB.m_trc, st));
        MMW_TRY(b_e2w.upload(HB.m_e2w, st));
        {   // slot of every association pair: the slot of its upper entry
            const size_t na = (size_t)H.E_asso();
            MMW_TRY(b_xasso.alloc(na));
            if (na) hipLaunchKernelGGL(k_gather_idx, dim3(grid_elems(na)), dim3(BLOCK), 0, st, na, d_apos, (const int*)b_e2w.p, b_xasso.p);
            MMW_HIP(hipGetLastError());
        }
        n_xs = (size_t)HB.m_nedges + (size_t)K;
        MMW_TRY(b_tmask.upload(HB.m_tmask, st));
        sddmm_mfma = true;
        return MMW_OK;
    }
    // ---- the argument structs of the blocked kernels
    BlkDev blkdev(int K, int Dpad, bool full_tile) const {
        BlkDev B;
        B.nb = HB.nb(); B.rowptr = b_rowptr.p; B.order = b_order.p; B.un_ptr = b_unptr.p; B.un_cols = b_uncols.p;
        B.bptr = b_bptr.p; B.lidx = b_lidx.p; B.self_li = b_selfli.p; B.desc = b_desc.p; B.un_fixed = b_unfixed.p;
        B.half_tile = HB.fits_half_tile && (double)K * Dpad * sizeof(T) < 4.0e9 && !full_tile;  // 32-bit byte offsets
        return B;
    }
    SdDev sd_dev() const {
        SdDev S;
        S.ptr = b_sdptr.p; S.la = b_sdla.p; S.lb = b_sdlb.p; S.epos = b_sdepos.p;
        return S;
    }
    Sd2Dev sd2_dev() const {
        Sd2Dev S;
        S.ptr = b_sd2ptr.p; S.ab = b_sd2ab.p; S.epos = b_sd2epos.p; S.items = b_sd2items.p; S.nitems = sd2_nitems;
        return S;
    }
    SdMfmaDev sd_mfma_dev() const {
        SdMfmaDev SM;
        SM.tbase = b_tbase.p; SM.tptr = b_tptr.p; SM.trc = b_trc.p; SM.nedges = (int)HB.m_nedges; SM.tmask = b_tmask.p;
        return SM;
    }
};
}  // namespace mmw
