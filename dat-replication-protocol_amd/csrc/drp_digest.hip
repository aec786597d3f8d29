// drp_digest.hip — gfx950 bucket digests of decoded Changes, for two stores that share no `change`
// counter (include/drp.h "digest / reconcile"): per bucket of identities the number of rows and the
// sum of their fingerprints (dig_cells), the buckets in which two such digests differ (dig_diff), and
// the count step of a select that keeps the rows of those buckets (dig_count; the scan and the scatter
// are drp_select.hip's).
// No reference counterpart: the reference has no relay; the fields read are those of
// messages/schema.proto:1-8.
//
// A row's identity hash is lat_group's and st_lookup's before the ctx's hash mask: XXH64 of the key,
// the subset's merged in. The mask never enters here, the cells cross the network. The fingerprint
// merges change, from, to, flags & (SUBSET | VALUE) and the value's XXH64 into it: what the store's
// `unchanged` rule compares. The candidates are the select's rows (sel_pred) whose key, subset and
// value ranges lie inside the wire (wire_has); no other row's bytes are read.
//   dig_cells   one row per lane, up to DIG_CHUNKS chunks of SEL_BLK rows per workgroup: predicate, bounds,
//               the three hashes, the fingerprint, then count += 1 and sum += fp in the row's cell.
//               A value of DIG_QUAD_MIN bytes or more is hashed by four adjacent lanes, one of
//               XXH64's four stripe accumulators each (dig_hash_quad), a shorter one by its row's lane.
//               Up to DIG_LDS_BITS bits the workgroup adds into a copy of the cells in LDS and, at
//               its end, adds its non-empty cells to the global ones (at bits = 0 every row of the
//               batch would otherwise hit one address); above, every row adds to the global cells
//               directly. All adds are relaxed atomics, workgroup scope in LDS and agent scope in
//               global memory. Addition commutes, so the cells are a function of the input; they are
//               complete at the kernel boundary, which is the only ordering used: no fence, no flag,
//               no lane waits for another, every loop is bounded (DESIGN.md "Latest per key").
//   dig_diff    one lane per bucket, the wave's ballot of "the two cells differ" as the set's word of
//               its 64 buckets, the popcounts added to *n_diff, one atomic per wave with a set bit.
//   dig_count   sel_count_kernel with the predicate "a candidate whose bucket's bit is set".
#include <algorithm>

#include "drp_select.h"

namespace drp {

constexpr uint32_t DIG_DIFF_BLK = 256;
// values from this length on are hashed by four lanes (dig_hash_quad): measured, a 64-byte value is
// hashed faster by its own lane (the shuffles and rounds cost more than two stripes), a 4 KB value by
// four (DESIGN.md "Digest")
constexpr uint32_t DIG_QUAD_MIN = 256;

// candidate row r's ranges (row_load: offsets absolute into the wire) lie inside the wire
__device__ __forceinline__ bool dig_in_wire(const RowSrc &S, const EncRow &r) {
  return wire_has(S, r.key_off, r.key_len) && (!(r.flags & DRP_F_SUBSET) || wire_has(S, r.subset_off, r.subset_len)) &&
         (!(r.flags & DRP_F_VALUE) || wire_has(S, r.value_off, r.value_len));
}

__device__ __forceinline__ uint64_t dig_ident(const RowSrc &S, const EncRow &r) {
  uint64_t h = xxh::xxh64(S.bytes + r.key_off, r.key_len);
  if (r.flags & DRP_F_SUBSET) h = xxh::merge(h, xxh::xxh64(S.bytes + r.subset_off, r.subset_len));
  return h;
}

// vhash: XXH64 of the value (read only with DRP_F_VALUE)
__device__ __forceinline__ uint64_t dig_fp(const EncRow &r, uint64_t ident, uint64_t vhash) {
  uint64_t h = xxh::merge(ident, r.change);
  h = xxh::merge(h, r.from);
  h = xxh::merge(h, r.to);
  h = xxh::merge(h, r.flags);  // (row_load masks them to SUBSET | VALUE)
  if (r.flags & DRP_F_VALUE) h = xxh::merge(h, vhash);
  return xxh::avalanche(h);
}

// XXH64 of the wire bytes [off, off + len) of every lane of the wave that sets `mine` (len >= 32;
// every lane calls this). A row gets four adjacent lanes, lane j of them stripe accumulator j (its
// eight bytes of every 32-byte stripe); sixteen rows a round, in lane order, at most four rounds.
// The first of the four lanes converges the accumulators and hashes the tail; the row's lane fetches
// the result. Only shuffles pass values between lanes. Returns the lane's own row's hash.
__device__ __forceinline__ uint64_t dig_hash_quad(const uint8_t *bytes, bool mine, uint64_t off, uint32_t len) {
  using ull = unsigned long long;
  const uint32_t lane = lane_id(), g = lane >> 2, j = lane & 3;
  uint64_t todo = __ballot(mine), out = 0;
  const uint32_t rank = (uint32_t)__popcll(todo & ((1ull << lane) - 1ull));  // among the wave's such rows
  for (uint32_t round = 0; round < 4 && todo; round++) {
    uint64_t t = todo;  // its lowest set bit: the lane of the row this lane's four take
    for (uint32_t q = 0; q < g; q++) t &= t - 1;
    const bool act = t != 0;
    const int src = act ? __builtin_ctzll(t) : 0;
    const uint64_t o = __shfl((ull)off, src, 64);
    const uint32_t n = (uint32_t)__shfl((int)len, src, 64);
    uint64_t v = xxh::acc0(j);
    if (act) {
      const uint8_t *p = bytes + o + 8 * j;
      uint32_t s = n >> 5;
      // eight stripes a step: their loads are issued before the first round waits for its word (one
      // load in flight per lane leaves the loop waiting on memory, stripe after stripe)
      for (; s >= 8; s -= 8, p += 256) {
        uint64_t w[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) w[k] = xxh::rd64(p + 32 * k);
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) v = xxh::round1(v, w[k]);
      }
      for (; s; s--, p += 32) v = xxh::round1(v, xxh::rd64(p));
    }
    const uint64_t v2 = __shfl_down((ull)v, 1, 64), v3 = __shfl_down((ull)v, 2, 64), v4 = __shfl_down((ull)v, 3, 64);
    uint64_t h = 0;
    if (act && j == 0) h = xxh::finish(xxh::converge(v, v2, v3, v4) + n, bytes + o + (n & ~31u), bytes + o + n);
    const uint64_t back = __shfl((ull)h, (int)((rank & 15) * 4), 64);
    if (mine && (rank >> 4) == round) out = back;
    for (uint32_t q = 0; q < 16; q++) todo &= todo - 1;
  }
  return out;
}

__device__ __forceinline__ uint32_t dig_bucket(uint64_t ident, uint32_t bits) {
  return bits ? (uint32_t)(ident >> (64 - bits)) : 0u;
}

__device__ __forceinline__ void dig_add(uint64_t *p, uint64_t v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(SEL_BLK) void dig_cells_kernel(const DigestParams D) {
  __shared__ drp_digest_cell lc[1u << DIG_LDS_BITS];
  __shared__ uint32_t ltot[2];
  const RowSrc &S = D.sel.src;
  const bool local = D.bits <= DIG_LDS_BITS;  // (uniform)
  const uint32_t ncell = 1u << D.bits;
  if (local)
    for (uint32_t b = threadIdx.x; b < ncell; b += SEL_BLK) lc[b] = drp_digest_cell{0, 0};
  if (threadIdx.x < 2) ltot[threadIdx.x] = 0;
  __syncthreads();
  uint32_t done = 0, left = 0;
  for (uint32_t k = 0; k < D.chunks; k++) {
    const uint64_t i = ((uint64_t)blockIdx.x * D.chunks + k) * SEL_BLK + threadIdx.x;
    EncRow r = {};
    bool cand = false;
    if (i < S.n && sel_pred(D.sel, i)) {
      r = row_load(S, i);
      cand = dig_in_wire(S, r);
      if (!cand) left++;
    }
    // the value's hash: a value of DIG_QUAD_MIN bytes or more with the wave, a shorter one by its lane
    const bool hv = cand && (r.flags & DRP_F_VALUE), wide = hv && r.value_len >= DIG_QUAD_MIN;
    uint64_t vhash = dig_hash_quad(S.bytes, wide, r.value_off, r.value_len);  // (every lane of the wave)
    if (hv && !wide) vhash = xxh::xxh64(S.bytes + r.value_off, r.value_len);
    if (!cand) continue;
    const uint64_t ident = dig_ident(S, r), fp = dig_fp(r, ident, vhash);
    const uint32_t b = dig_bucket(ident, D.bits);
    done++;
    if (local) {
      __hip_atomic_fetch_add(&lc[b].count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&lc[b].sum, fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      dig_add(&D.cells[b].count, 1);
      dig_add(&D.cells[b].sum, fp);
    }
  }
  if (D.totals) {
    done = wave_sum32(done);
    left = wave_sum32(left);
    if (lane_id() == 0) {
      if (done) atomicAdd(&ltot[0], done);
      if (left) atomicAdd(&ltot[1], left);
    }
  }
  __syncthreads();
  if (local)
    for (uint32_t b = threadIdx.x; b < ncell; b += SEL_BLK) {
      const drp_digest_cell c = lc[b];
      if (c.count) {  // (a cell with no row has sum 0)
        dig_add(&D.cells[b].count, c.count);
        dig_add(&D.cells[b].sum, c.sum);
      }
    }
  if (D.totals && threadIdx.x < 2 && ltot[threadIdx.x]) dig_add(&D.totals[threadIdx.x], ltot[threadIdx.x]);
}

__global__ __launch_bounds__(DIG_DIFF_BLK) void dig_diff_kernel(const drp_digest_cell *a, const drp_digest_cell *b,
                                                                uint32_t ncell, uint64_t *bucket_set, uint64_t *n_diff) {
  const uint32_t i = blockIdx.x * DIG_DIFF_BLK + threadIdx.x;
  bool differs = false;
  if (i < ncell) {
    const drp_digest_cell x = a[i], y = b[i];
    differs = x.count != y.count || x.sum != y.sum;
  }
  const uint64_t w = __ballot(differs);
  // (the wave's first bucket i names the set's word i >> 6; with ncell < 64 only the first wave has one,
  // and its lanes from ncell on have voted 0)
  if (lane_id() == 0 && i < ncell) {
    bucket_set[i >> 6] = w;
    if (w) dig_add(n_diff, (uint64_t)__popcll(w));
  }
}

__global__ __launch_bounds__(SEL_BLK) void dig_count_kernel(const DigestParams D) {
  const RowSrc &S = D.sel.src;
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  bool keep = false;
  if (i < S.n && sel_pred(D.sel, i)) {
    const EncRow r = row_load(S, i);
    if (dig_in_wire(S, r)) {
      const uint32_t b = dig_bucket(dig_ident(S, r), D.bits);
      keep = (D.bucket_set[b >> 6] >> (b & 63)) & 1ull;
    }
  }
  sel_publish(D.sel, keep);
}

}  // namespace drp

using namespace drp;

extern "C" hipError_t drp_launch_digest(const DigestParams *Dp, const SelectBytes *fb, void *scratch, hipStream_t st) {
  DigestParams D = *Dp;
  if (const hipError_t e = hipMemsetAsync(D.cells, 0, sizeof(drp_digest_cell) << D.bits, st)) return e;
  if (D.totals)
    if (const hipError_t e = hipMemsetAsync(D.totals, 0, 16, st)) return e;
  const uint64_t n = D.sel.src.n, nchunk = (n + SEL_BLK - 1) / SEL_BLK;
  if (!n) return hipSuccess;
  D.chunks = (uint32_t)std::min<uint64_t>(DIG_CHUNKS, std::max<uint64_t>(1, nchunk / DIG_GRID_MIN));
  const uint64_t nblk = (nchunk + D.chunks - 1) / D.chunks;
  // (only the filter's byte strings are placed: dig_cells reads neither ballot words nor counts)
  if (const hipError_t e = drp_select_place(&D.sel, fb, scratch, st)) return e;
  hipLaunchKernelGGL(dig_cells_kernel, dim3((uint32_t)nblk), dim3(SEL_BLK), 0, st, D);
  drp_dbg_mark("digest", st);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_digest_diff(const drp_digest_cell *a, const drp_digest_cell *b, uint32_t bits,
                                             uint64_t *bucket_set, uint64_t *n_diff, hipStream_t st) {
  if (const hipError_t e = hipMemsetAsync(n_diff, 0, 8, st)) return e;
  const uint32_t ncell = 1u << bits;
  hipLaunchKernelGGL(dig_diff_kernel, dim3((ncell + DIG_DIFF_BLK - 1) / DIG_DIFF_BLK), dim3(DIG_DIFF_BLK), 0, st, a, b,
                     ncell, bucket_set, n_diff);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_select_buckets(const DigestParams *Dp, const SelectBytes *fb, void *scratch,
                                                hipStream_t st) {
  DigestParams D = *Dp;
  const uint64_t n = D.sel.src.n;
  if (n == 0) return hipMemsetAsync(D.sel.n_selected, 0, 8, st);
  if (const hipError_t e = drp_select_place(&D.sel, fb, scratch, st)) return e;
  hipLaunchKernelGGL(dig_count_kernel, dim3((uint32_t)((n + SEL_BLK - 1) / SEL_BLK)), dim3(SEL_BLK), 0, st, D);
  const hipError_t e = drp_launch_select_compact(&D.sel, st);  // (the last error of all the launches)
  drp_dbg_mark("select_buckets", st);
  return e;
}
