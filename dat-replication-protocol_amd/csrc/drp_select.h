// drp_select.h — the select predicate over the decoded Change columns, shared by the kernels that
// evaluate it (drp_select.hip, drp_latest.hip), and the geometry of the stable compaction both end in.
#pragma once
#include "drp_device.h"
#include "drp_kernels.h"

namespace drp {

constexpr uint32_t SEL_BLK = 1024, SEL_WAVES = SEL_BLK / 64;

// what row i's payload offsets lack to be offsets into P.bytes
__device__ __forceinline__ uint64_t sel_shift(const SelectParams &P, uint64_t i) {
  if (P.npieces <= 1) return P.shift0;
  uint64_t lo = 0, hi = P.npieces;  // piece_row[lo] <= i < piece_row[hi]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (P.piece_row[mid] <= i) lo = mid;
    else hi = mid;
  }
  return P.piece_shift[lo];
}

// wire bytes [off, off + len) == ref[0, len); a range outside the wire matches nothing
__device__ __forceinline__ bool sel_bytes_eq(const SelectParams &P, uint64_t off, uint32_t len, const uint8_t *ref) {
  if ((uint64_t)len > P.nbytes || off > P.nbytes - len) return false;
  const uint8_t *w = P.bytes + off;
  for (uint32_t k = 0; k < len; k++)
    if (w[k] != ref[k]) return false;
  return true;
}

__device__ __forceinline__ bool sel_pred(const SelectParams &P, uint64_t i) {
  const drp_changes &c = P.cols;
  if ((P.type[i] & 0x3F) != DRP_TYPE_CHANGE) return false;
  const uint32_t fl = c.flags[i];
  if (fl & DRP_F_BAD) return false;
  const uint32_t ff = P.fflags;
  if (ff & DRP_SEL_CHANGE_RANGE) {
    const uint64_t v = c.change[i];
    if (v < P.change_min || v > P.change_max) return false;
  }
  if ((ff & DRP_SEL_SUBSET_NONE) && (fl & DRP_F_SUBSET)) return false;
  if (ff & DRP_SEL_SUBSET_EQ) {
    if (!(fl & DRP_F_SUBSET) || c.subset_len[i] != P.subset_len) return false;
  }
  if ((ff & DRP_SEL_KEY_PREFIX) && c.key_len[i] < P.prefix_len) return false;
  // the byte compares last: only rows whose lengths match read the wire
  if ((ff & DRP_SEL_SUBSET_EQ) && P.subset_len) {
    const uint64_t off = P.payload_off[i] + sel_shift(P, i) + c.subset_off[i];
    if (!sel_bytes_eq(P, off, P.subset_len, P.subset)) return false;
  }
  if ((ff & DRP_SEL_KEY_PREFIX) && P.prefix_len) {
    const uint64_t off = P.payload_off[i] + sel_shift(P, i) + c.key_off[i];
    if (!sel_bytes_eq(P, off, P.prefix_len, P.prefix)) return false;
  }
  return true;
}

}  // namespace drp
