// drp_select.h — what the relay kernels share (drp_select.hip, drp_latest.hip, drp_fanout.hip), one
// copy each: where a row's bytes lie in the wire (row_shift) and whether a range lies in it (wire_has,
// wire_eq), the filter predicate (pred_load, pred_conds; sel_pred for one filter), the copy of a row
// into encoder rows (row_load, row_store), and the geometry and epilogue (sel_publish) of the count
// step that the select's stable compaction starts from.
#pragma once
#include "drp_device.h"
#include "drp_kernels.h"

namespace drp {

constexpr uint32_t SEL_BLK = 1024, SEL_WAVES = SEL_BLK / 64;
// the fan-out's count geometry (drp_fanout.hip; drp_latest.hip rewrites its planes and counts): a
// workgroup of 16 waves takes FAN_ROWS = 4096 rows, wave w the 64-row chunks 4w .. 4w + 3
constexpr uint32_t FAN_BLK = 1024, FAN_WAVES = FAN_BLK / 64, FAN_RPL = 4;
constexpr uint32_t FAN_ROWS = FAN_BLK * FAN_RPL, FAN_CHUNKS = FAN_ROWS / 64;  // 64 ballot words per workgroup

// what row i's payload offsets lack to be offsets into S.bytes
__device__ __forceinline__ uint64_t row_shift(const RowSrc &S, uint64_t i) {
  if (S.npieces <= 1) return S.shift0;
  uint64_t lo = 0, hi = S.npieces;  // piece_row[lo] <= i < piece_row[hi]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (S.piece_row[mid] <= i) lo = mid;
    else hi = mid;
  }
  return S.piece_shift[lo];
}

// [off, off + len) lies inside the wire: a range that does not is never read and matches nothing
__device__ __forceinline__ bool wire_has(const RowSrc &S, uint64_t off, uint32_t len) {
  return (uint64_t)len <= S.nbytes && off <= S.nbytes - len;
}

// wire bytes [off, off + len) == ref[0, len)
__device__ __forceinline__ bool wire_eq(const RowSrc &S, uint64_t off, uint32_t len, const uint8_t *ref) {
  if (!wire_has(S, off, len)) return false;
  const uint8_t *w = S.bytes + off;
  for (uint32_t k = 0; k < len; k++)
    if (w[k] != ref[k]) return false;
  return true;
}

// x[0, len) == y[0, len) (any alignment; both ranges readable)
__device__ __forceinline__ bool bytes_eq(const uint8_t *x, const uint8_t *y, uint32_t len) {
  if (len < 8) {
    for (uint32_t k = 0; k < len; k++)
      if (x[k] != y[k]) return false;
    return true;
  }
  // eight bytes per step (unaligned 8-byte loads), the last step over the last eight bytes
  for (uint32_t k = 0; k + 8 < len; k += 8)
    if (xxh::rd64(x + k) != xxh::rd64(y + k)) return false;
  return xxh::rd64(x + len - 8) == xxh::rd64(y + len - 8);
}

// the columns of one row the predicate reads (loaded once, whatever the number of filters)
struct PredRow {
  uint64_t change, sub_at, key_at;  // sub_at / key_at: the subset's / key's offset into S.bytes
  uint32_t flags, subset_len, key_len;
};

// r's columns of row i, a well-formed Change (r.flags is set already): only those the conditions
// `flags` name, and the offsets only of the byte strings `bytes` says are compared (filter_bytes)
__device__ __forceinline__ void pred_load(const RowSrc &S, uint64_t i, uint32_t flags, uint32_t bytes, PredRow &r) {
  const drp_changes &c = S.cols;
  if (flags & DRP_SEL_CHANGE_RANGE) r.change = c.change[i];
  if (flags & DRP_SEL_SUBSET_EQ) r.subset_len = c.subset_len[i];
  if (flags & DRP_SEL_KEY_PREFIX) r.key_len = c.key_len[i];
  if (bytes) {
    const uint64_t base = S.payload_off[i] + row_shift(S, i);
    if (bytes & DRP_SEL_SUBSET_EQ) r.sub_at = base + c.subset_off[i];
    if (bytes & DRP_SEL_KEY_PREFIX) r.key_at = base + c.key_off[i];
  }
}

// the filter's conditions on a loaded row, the byte compares last: only rows whose lengths match
// read the wire
__device__ __forceinline__ bool pred_conds(const RowSrc &S, const RowFilter &F, const uint8_t *subset,
                                           const uint8_t *prefix, const PredRow &r) {
  const uint32_t ff = F.flags;
  if ((ff & DRP_SEL_CHANGE_RANGE) && (r.change < F.change_min || r.change > F.change_max)) return false;
  if ((ff & DRP_SEL_SUBSET_NONE) && (r.flags & DRP_F_SUBSET)) return false;
  if ((ff & DRP_SEL_SUBSET_EQ) && (!(r.flags & DRP_F_SUBSET) || r.subset_len != F.subset_len)) return false;
  if ((ff & DRP_SEL_KEY_PREFIX) && r.key_len < F.prefix_len) return false;
  if ((ff & DRP_SEL_SUBSET_EQ) && F.subset_len && !wire_eq(S, r.sub_at, F.subset_len, subset)) return false;
  if ((ff & DRP_SEL_KEY_PREFIX) && F.prefix_len && !wire_eq(S, r.key_at, F.prefix_len, prefix)) return false;
  return true;
}

// the select's one filter on row i
__device__ __forceinline__ bool sel_pred(const SelectParams &P, uint64_t i) {
  const RowSrc &S = P.src;
  if ((S.type[i] & 0x3F) != DRP_TYPE_CHANGE) return false;
  PredRow r = {};
  r.flags = S.cols.flags[i];
  if (r.flags & DRP_F_BAD) return false;
  pred_load(S, i, P.f.flags, filter_bytes(P.f), r);
  return pred_conds(S, P.f, P.subset, P.prefix, r);
}

// the count step's epilogue (one row per lane): the wave's ballot of `keep` as the ballot word of
// its 64 rows, the popcounts summed across the workgroup's waves in LDS into its count
__device__ __forceinline__ void sel_publish(const SelectParams &P, bool keep) {
  __shared__ uint32_t wcnt[SEL_WAVES];
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  const uint64_t b = __ballot(keep);
  if (lane_id() == 0) {
    P.mask[i >> 6] = b;  // (i >> 6 < ceil(n / 64) rounded up to the workgroup: the scratch covers it)
    wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < SEL_WAVES; k++) s += wcnt[k];
    P.block_cnt[blockIdx.x] = s;
  }
}

// a row as the encoder takes it: offsets absolute into the wire
struct EncRow {
  uint64_t key_off, subset_off, value_off, change, from, to;
  uint32_t key_len, subset_len, value_len;
  uint8_t flags;
};

__device__ __forceinline__ EncRow row_load(const RowSrc &S, uint64_t i) {
  const drp_changes &c = S.cols;
  const uint64_t at = S.payload_off[i] + row_shift(S, i);
  EncRow r;
  r.key_off = at + c.key_off[i];
  r.key_len = c.key_len[i];
  r.subset_off = at + c.subset_off[i];
  r.subset_len = c.subset_len[i];
  r.value_off = at + c.value_off[i];
  r.value_len = c.value_len[i];
  r.change = c.change[i];
  r.from = c.from[i];
  r.to = c.to[i];
  r.flags = (uint8_t)(c.flags[i] & (DRP_F_SUBSET | DRP_F_VALUE));  // (no key-post bit reaches the encoder)
  return r;
}

// source row i's values to slot `slot` of the output
__device__ __forceinline__ void row_store(const RowOut &O, uint64_t slot, const EncRow &r, uint64_t i) {
  O.o_key_off[slot] = r.key_off;
  O.o_key_len[slot] = r.key_len;
  O.o_subset_off[slot] = r.subset_off;
  O.o_subset_len[slot] = r.subset_len;
  O.o_value_off[slot] = r.value_off;
  O.o_value_len[slot] = r.value_len;
  O.o_change[slot] = r.change;
  O.o_from[slot] = r.from;
  O.o_to[slot] = r.to;
  O.o_flags[slot] = r.flags;
  if (O.sel_idx) O.sel_idx[slot] = i;
}

}  // namespace drp
