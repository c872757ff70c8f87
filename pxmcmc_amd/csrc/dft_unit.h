// Host interface of the pair and quad units (dft_wave.hip) behind the dispatcher of dft.hip (sht_core.h: make_dft_plan, launch_*).  Only the
// DFT sources include this header.
#pragma once
#include "sht_core.h"

namespace pxm {

// pair unit (dft_wave.hip): n <= 511
int pair_r0(int n);  // Mh / 64 for ring length n, 0 = not covered (n > 512)
// the workgroup of a ring length the pair unit covers, on ring arrays of whole lines (ncol >= 8): rings per workgroup, threads, LDS
// bytes and whether the exact-length body runs (n = 511 and pfa)
void pair_workgroup(int n, bool pfa, int* rings, int* threads, size_t* lds, bool* exact);
int pair_make_tables(int n, bool pfa, PairTables* t);  // pfa: n = 511 also gets the tables of the exact-length body
int pair_px2ring(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t st);
int pair_ring2px(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t st, bool ring_out);

// quad unit (dft_wave.hip): 511 < n <= 1023
void quad_workgroup(int* chains, int* threads, size_t* lds);  // of a launch with more than one chain (one chain: a workgroup of four waves)
int quad_make_tables(int n, QuadTables* t);
int quad_px2ring(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t st);
int quad_ring2px(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t st);

}  // namespace pxm
