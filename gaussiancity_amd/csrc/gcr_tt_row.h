// gcr_tt_row.h -- which row of the tile table belongs to workgroup b of the tile-table kernels (gcr_binning.hip)?
//
// base[row][t], the column prefix over the table's rows, decides where a workgroup's keys land inside tile t's segment
// of `pairs`: the rows in order, one run of keys each.  With row = b, the ~18 keys the workgroups of one XCD add to a
// 145-key segment lie spread over the whole segment -- workgroups are dealt to the eight XCDs round-robin, so b, b + 8,
// b + 16 ... share an L2 and nobody else does -- and each L2 holds a share of nearly every cache line of `pairs`, partly
// dirty, until it evicts the line partly filled.  gcr_tt_row() lays the rows out XCD CLASS BY XCD CLASS instead: all b with
// the same b % 8 in consecutive rows, so that the keys one L2 sees of a segment are one contiguous run.
//
//   base(c) = c * (NG / 8) + min(c, NG % 8)     rows in front of class c (the first NG % 8 classes hold one more)
//   row(b)  = base(b % 8) + b / 8               a bijection of [0, NG) for every NG >= 1
//
// That workgroup b runs on XCD b % 8 is a SPEED assumption only (a dispatch order the hardware does not promise): under
// any other placement the stores merge as badly as before and nothing else changes.  Correctness rests on the slot order
// inside a tile segment being unobservable -- the keys are unique (depth, index) pairs and the tile sort orders them
// (gcr_binning.hip, comment above RANK_MERGE_MAX) -- and on both instantiations of k_tile_table using the same row.
//
// The header compiles on the host too (tests/test_tt_row_host.py checks the bijection for every NG with gcc).
#pragma once

#if defined(__HIPCC__)
#define GCR_TT_ROW_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GCR_TT_ROW_FN static inline
#endif

#define GCR_XCDS 8  // L2s the workgroups of a grid are dealt over

GCR_TT_ROW_FN unsigned gcr_tt_row(unsigned b, unsigned NG) {
  const unsigned c = b % GCR_XCDS, q = NG / GCR_XCDS, r = NG % GCR_XCDS;
  return c * q + (c < r ? c : r) + b / GCR_XCDS;
}
