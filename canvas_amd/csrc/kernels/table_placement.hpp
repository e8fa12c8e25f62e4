// table_placement.hpp -- where the 128 KiB half -> half table of a Y'CbCr edge kernel lives, and the persistent launch that goes
// with it: k_mpeg2_subsample, k_mpeg2_reconstruct, k_ycc422_subsample, k_ycc422_reconstruct, k_ycc420_subsample and
// k_ycc420_reconstruct (what else those six share: ycc_edge.hpp).  color_ops.hip / chain_kernel.hpp keep table copies of their own,
// shaped by those kernels' pipelining.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace cvs {

constexpr int kTable = 65536;          // entries: one per half code
// Staged into LDS by 1024-lane workgroups, one per CU (the table fills the LDS), or gathered from L2 through the vector L1 by
// 256-lane workgroups, six per CU.  Or absent (the 4:2:0 edges without a transfer curve): launched like the gathered form.
// kTableLdsUnstaged is the diagnostic build's LDS form without the staging copy (k_mpeg2_subsample, timing only: its pixels are
// wrong), which isolates what the staging costs.
enum { kTableLds = 0, kTableL2 = 1, kTableNone = 2, kTableLdsUnstaged = 3 };
constexpr int kTableLdsLanes = 1024, kTableL2Lanes = 256, kTableL2PerCu = 6;
// Chosen by measurement (profiles/mpeg2): staging costs every workgroup ~2 us before its first pixel, which a small raster does
// not earn back.  Kernel medians gathering vs staged, us:
//                  k_mpeg2_subsample    k_mpeg2_reconstruct, interlaced (profiles/mpeg2/recon_*)
//   720x480          4.4 vs  8.1                          4.9 vs  8.1
//   1920x1080       12.9 vs 11.3                         12.5 vs  9.5
//   3840x2160       37.2 vs 22.3                         42.7 vs 22.4
// The switch sits between the two smaller measured sizes, at one megapixel, for both.
constexpr long long kGatherUpTo = 1LL << 20;

// the placement for a raster; the diagnostic build takes CVS_MPEG2_TABLE instead, whatever number it holds
inline int table_placement(long long pixels) {
    if (const char *e = CVS_DIAG_ENV("CVS_MPEG2_TABLE")) return atoi(e);
    return pixels <= kGatherUpTo ? kTableL2 : kTableLds;
}

// the staging copy, 16 bytes per lane and trip; the caller's __syncthreads() ends it
template <int LANES>
__device__ __forceinline__ void stage_table(uint16_t *lds, const uint16_t *lut) {
    const uint4 *src = reinterpret_cast<const uint4 *>(lut);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (int i = threadIdx.x; i < kTable * 2 / 16; i += LANES) dst[i] = src[i];
}

// the persistent launch: workgroups of this many lanes, at most this many of them on `cus` CUs ...
inline bool table_in_lds(int table) { return table == kTableLds || table == kTableLdsUnstaged; }
inline long long table_lanes(int table) { return table_in_lds(table) ? kTableLdsLanes : kTableL2Lanes; }
inline long long table_workgroups(int table, long long cus) { return table_in_lds(table) ? cus : cus * kTableL2PerCu; }
// ... and no workgroup without a unit of work of its own (one unit per wave and trip)
template <int LANES>
inline dim3 table_grid(long long units, long long most) {
    const long long want = (units + LANES / 64 - 1) / (LANES / 64);
    return dim3((unsigned)(want < most ? want : most));
}

}  // namespace cvs
