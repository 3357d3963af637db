// How a kernel walks an int32 label plane to make a per-label table: what
// k_object_table (objects_kernels.hip) and k_intensity_table
// (measure_kernels.hip) share.  Included by those two only.
//
// A label plane is mostly runs of equal labels along a row, and one atomic per
// pixel would run at the atomic rate, not HBM's.  So:
//  * a workgroup of kTileWaves waves owns a tile of kTileRows x kTileCols
//    pixels, walked as kTileItems items of 64 consecutive pixels of a row; wave
//    wv takes items wv, wv + kTileWaves, ... (tile_item);
//  * the runs of an item are found with one shuffle and one ballot: run heads
//    are the lanes whose label differs from the lower lane's (label_runs).  One
//    lane per run then acts for it, with the run's totals;
//  * that lane updates a per-workgroup table in LDS, not memory: a tile meets a
//    few dozen to a few hundred labels, and each used entry is flushed once, so
//    memory sees one set of atomics per (label, tile) instead of per run.  The
//    table is open addressing on the label (label_slot).  A label that finds
//    no entry within the probe limit (a tile with more labels than the table
//    holds) updates memory directly: slower, still exact.
// Everything is an integer atomic, so a table is exact and the same bytes from
// call to call.  Labels outside [0, max_label] are never written: the C-ABI
// rejects such a plane from k_label_minmax's result before a table kernel is
// launched, and the kernels skip them on their own as well.
#pragma once

#include "common.h"

namespace tmh {

constexpr int kTileRows = 16, kTileCols = 512;  // a workgroup's tile
constexpr int kTileSegs = kTileCols / 64, kTileItems = kTileRows * kTileSegs;
constexpr int kTileWaves = 4;

// a lane's pixel of item i of the tile at (r0, c0): row r0 + i / kTileSegs,
// columns c0 + 64 (i % kTileSegs) ..; the valid lanes of an item are lanes
// 0 .. nv - 1
struct TileItem {
  int y, x;
  bool valid;
};

__device__ __forceinline__ TileItem tile_item(int i, int r0, int c0, int lane, int H, int W) {
  const int y = r0 + i / kTileSegs, x = c0 + (i % kTileSegs) * 64 + lane;
  return {y, x, i < kTileItems && y < H && x < W};
}

// the runs of equal labels among an item's valid lanes: whether this lane is a
// run's first, the wave's head lanes and the number of valid lanes.  All 64
// lanes must be active.
struct LabelRuns {
  bool head;
  unsigned long long heads;
  int nv;
};

__device__ __forceinline__ LabelRuns label_runs(int L, bool valid, int lane) {
  const int below = __shfl_up(L, 1, 64);
  const bool head = valid && (lane == 0 || L != below);
  return {head, __ballot(head), (int)__popcll(__ballot(valid))};
}

// The entry of a tile's table (512 labels, -1 where free) at which the probes
// for label L begin: the top 9 bits of L * 2654435761 mod 2^32.  From there a
// kernel probes linearly, claims a free entry with atomicCAS and gives up
// after its probe limit.  That loop stands in each kernel, not here: the
// compiler optimises a function on its own before it inlines it, which gives
// the loop other instructions than it has inside the kernels (a found flag
// and a break: 16 unrolled probes; held rolled: another exit test), and that
// form was slower than the kernels' own in two one-channel cases of
// tools/bench_measure.py (profiles/r23/ab_label_claim_r23.txt).
static_assert(TMH_OBJECT_SLOTS == 512, "the hash keeps 9 bits");
static_assert(TMH_OBJECT_PROBE >= 1 && TMH_OBJECT_PROBE < TMH_OBJECT_SLOTS,
              "a probe sequence stays inside the table");
// the tests take the labels of their probe-limit cases from one statement of
// this rule for both tables
static_assert(TMH_OBJECT_SLOTS == TMH_INTENSITY_SLOTS && TMH_OBJECT_PROBE == TMH_INTENSITY_PROBE,
              "both tables hash and probe alike");

__device__ __forceinline__ int label_slot(int L) {
  return (int)(((unsigned int)L * 2654435761u) >> 23);
}

}  // namespace tmh
