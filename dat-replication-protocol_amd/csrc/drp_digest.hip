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
//               its 64 buckets, the popcounts summed over the workgroup's waves and runs in LDS and added
//               to *n_diff, one atomic per workgroup with a set bit. Any cell count: the second level's
//               cells are compared by the same kernel, a workgroup then taking several runs of cells.
//   dig_count   sel_count_kernel with the predicate "a candidate whose bucket's bit is set".
// The second level inside the buckets of a set (dig_rank, dig_zero, dig_refine, dig_count2) is below.
#include <algorithm>

#include "drp_select.h"

namespace drp {

constexpr uint32_t DIG_DIFF_BLK = 256, DIG_DIFF_STEPS = 16, DIG_DIFF_GRID_MIN = 2048;
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
                                                                uint32_t ncell, uint64_t *bucket_set, uint64_t *n_diff,
                                                                uint32_t steps) {
  __shared__ uint32_t wcnt[DIG_DIFF_BLK / 64];
  uint32_t cnt = 0;  // (the wave's first lane: the set bits of its words)
  for (uint32_t k = 0; k < steps; k++) {
    const uint32_t i = (blockIdx.x * steps + k) * DIG_DIFF_BLK + threadIdx.x;  // (< 2^24 + steps * DIG_DIFF_BLK)
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
      cnt += (uint32_t)__popcll(w);
    }
  }
  // one add per workgroup: with many cells differing, one per wave to the one address was the kernel's time
  if (lane_id() == 0) wcnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < DIG_DIFF_BLK / 64; q++) s += wcnt[q];
    if (s) dig_add(n_diff, (uint64_t)s);
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

// ---- the second level: cells inside the buckets of a set (include/drp.h "refined digests") ----------
//   dig_rank    one workgroup, one word of the bucket set per lane: the exclusive prefix of the words'
//               popcounts (a wave scan, the waves' sums through LDS) as the rank table, their sum
//               (n_set) to totals[2]; totals[0] and [1] are cleared here, for dig_refine's adds.
//   dig_zero    cells2[0, n_set << sub_bits) cleared, if that many fit cells_cap: the launcher cannot
//               know n_set, so the grid is sized from the bound it does know and strides.
//   dig_refine  dig_cells over the candidates whose bucket's bit is set, into cell
//               slot(bucket) << sub_bits | sub. Predicate, bounds and the identity hash for every
//               selected row, the value's hash only for members (and only if the cells fit: the
//               verdict is taken from n_set, uniformly). Up to DIG_REFINE_LDS_CELLS cells the
//               workgroup sums into a copy in LDS, as dig_cells does.
//   dig_count2  dig_count with the second test: the bit of the row's cell in cell_set.
// The same discipline: relaxed atomic adds only, the kernel boundary the only ordering.
__device__ __forceinline__ uint32_t dig_sub(uint64_t ident, uint32_t bits, uint32_t sub_bits) {
  return (uint32_t)(ident >> (64 - bits - sub_bits)) & ((1u << sub_bits) - 1u);  // (bits + sub_bits <= 24)
}

// bucket b's bit in the set and, if it is set, the row's cell: slot(b) << sub_bits | sub
__device__ __forceinline__ bool dig_cell2(const RefineParams &R, uint64_t ident, uint32_t &cell) {
  const uint32_t b = dig_bucket(ident, R.d.bits);
  const uint64_t word = R.d.bucket_set[b >> 6];
  if (!((word >> (b & 63)) & 1ull)) return false;
  const uint32_t slot = R.rank[b >> 6] + (uint32_t)__popcll(word & ((1ull << (b & 63)) - 1ull));
  cell = (slot << R.sub_bits) | dig_sub(ident, R.d.bits, R.sub_bits);
  return true;
}

// mask0: the bits of word 0 that name buckets (all of them from bits = 6 on)
__global__ __launch_bounds__(DIG_RANK_BLK) void dig_rank_kernel(const uint64_t *set, uint32_t nwords, uint64_t mask0,
                                                                uint32_t *rank, uint64_t *totals) {
  __shared__ uint32_t wsum[DIG_RANK_BLK / 64];
  const uint32_t t = threadIdx.x;
  const uint32_t pc = t < nwords ? (uint32_t)__popcll(set[t] & (t ? ~0ull : mask0)) : 0u;
  uint32_t all;
  const uint32_t before = block_excl_scan(pc, wsum, all);
  if (t < nwords) rank[t] = before;
  if (t == 0 && totals) {
    totals[0] = 0;
    totals[1] = 0;
    totals[2] = all;
  }
}

__global__ __launch_bounds__(DIG_DIFF_BLK) void dig_zero_kernel(drp_digest_cell *cells, uint64_t cells_cap, uint32_t sub_bits,
                                                                const uint64_t *totals) {
  const uint64_t ncell = totals[2] << sub_bits;
  if (ncell > cells_cap) return;
  for (uint64_t c = (uint64_t)blockIdx.x * DIG_DIFF_BLK + threadIdx.x; c < ncell; c += (uint64_t)gridDim.x * DIG_DIFF_BLK)
    cells[c] = drp_digest_cell{0, 0};
}

__global__ __launch_bounds__(SEL_BLK) void dig_refine_kernel(const RefineParams R) {
  __shared__ drp_digest_cell lc[DIG_REFINE_LDS_CELLS];
  __shared__ uint32_t ltot[2];
  const DigestParams &D = R.d;
  const RowSrc &S = D.sel.src;
  const uint64_t ncell = uniform64(D.totals[2]) << R.sub_bits;  // (dig_rank's n_set: no workgroup writes it)
  const bool fits = ncell <= R.cells_cap;
  const bool local = fits && ncell <= DIG_REFINE_LDS_CELLS;
  if (local)
    for (uint32_t c = threadIdx.x; c < ncell; c += SEL_BLK) lc[c] = drp_digest_cell{0, 0};
  if (threadIdx.x < 2) ltot[threadIdx.x] = 0;
  __syncthreads();
  uint32_t done = 0, left = 0;
  for (uint32_t k = 0; k < D.chunks; k++) {
    const uint64_t i = ((uint64_t)blockIdx.x * D.chunks + k) * SEL_BLK + threadIdx.x;
    EncRow r = {};
    bool member = false;
    uint64_t ident = 0;
    uint32_t cell = 0;
    if (i < S.n && sel_pred(D.sel, i)) {
      r = row_load(S, i);
      if (dig_in_wire(S, r)) {
        ident = dig_ident(S, r);
        member = dig_cell2(R, ident, cell);
      } else {
        left++;
      }
    }
    // only a member's value is read, and none if the cells do not fit: the totals need no fingerprint
    const bool hv = member && fits && (r.flags & DRP_F_VALUE), wide = hv && r.value_len >= DIG_QUAD_MIN;
    uint64_t vhash = dig_hash_quad(S.bytes, wide, r.value_off, r.value_len);  // (every lane of the wave)
    if (hv && !wide) vhash = xxh::xxh64(S.bytes + r.value_off, r.value_len);
    if (!member) continue;
    done++;
    if (!fits) continue;
    const uint64_t fp = dig_fp(r, ident, vhash);
    if (local) {
      __hip_atomic_fetch_add(&lc[cell].count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(&lc[cell].sum, fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      dig_add(&D.cells[cell].count, 1);
      dig_add(&D.cells[cell].sum, fp);
    }
  }
  done = wave_sum32(done);
  left = wave_sum32(left);
  if (lane_id() == 0) {
    if (done) atomicAdd(&ltot[0], done);
    if (left) atomicAdd(&ltot[1], left);
  }
  __syncthreads();
  if (local)
    for (uint32_t c = threadIdx.x; c < ncell; c += SEL_BLK) {
      const drp_digest_cell v = lc[c];
      if (v.count) {  // (a cell with no row has sum 0)
        dig_add(&D.cells[c].count, v.count);
        dig_add(&D.cells[c].sum, v.sum);
      }
    }
  if (threadIdx.x < 2 && ltot[threadIdx.x]) dig_add(&D.totals[threadIdx.x], ltot[threadIdx.x]);
}

__global__ __launch_bounds__(SEL_BLK) void dig_count2_kernel(const RefineParams R) {
  const RowSrc &S = R.d.sel.src;
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  bool keep = false;
  if (i < S.n && sel_pred(R.d.sel, i)) {
    const EncRow r = row_load(S, i);
    uint32_t cell = 0;
    if (dig_in_wire(S, r) && dig_cell2(R, dig_ident(S, r), cell)) keep = (R.cell_set[cell >> 6] >> (cell & 63)) & 1ull;
  }
  sel_publish(R.d.sel, keep);
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

extern "C" hipError_t drp_launch_digest_diff_cells(const drp_digest_cell *a, const drp_digest_cell *b, uint32_t ncell,
                                                   uint64_t *cell_set, uint64_t *n_diff, hipStream_t st) {
  if (const hipError_t e = hipMemsetAsync(n_diff, 0, 8, st)) return e;
  if (!ncell) return hipMemsetAsync(cell_set, 0, 8, st);  // (no wave names the one word)
  // a workgroup takes up to DIG_DIFF_STEPS runs of DIG_DIFF_BLK cells, but no more than leave DIG_DIFF_GRID_MIN
  // workgroups (one run each up to 2^19 cells: every first-level digest)
  const uint32_t nrun = (ncell + DIG_DIFF_BLK - 1) / DIG_DIFF_BLK;
  const uint32_t steps = std::min(DIG_DIFF_STEPS, std::max(1u, nrun / DIG_DIFF_GRID_MIN));
  hipLaunchKernelGGL(dig_diff_kernel, dim3((nrun + steps - 1) / steps), dim3(DIG_DIFF_BLK), 0, st, a, b, ncell, cell_set,
                     n_diff, steps);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_digest_diff(const drp_digest_cell *a, const drp_digest_cell *b, uint32_t bits,
                                             uint64_t *bucket_set, uint64_t *n_diff, hipStream_t st) {
  return drp_launch_digest_diff_cells(a, b, 1u << bits, bucket_set, n_diff, st);
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

static void dig_launch_rank(const RefineParams &R, uint64_t *totals, hipStream_t st) {
  const uint64_t mask0 = R.d.bits < 6 ? (1ull << (1u << R.d.bits)) - 1ull : ~0ull;
  hipLaunchKernelGGL(dig_rank_kernel, dim3(1), dim3(DIG_RANK_BLK), 0, st, R.d.bucket_set, R.set_words, mask0, R.rank,
                     totals);
}

extern "C" hipError_t drp_launch_digest_refine(const RefineParams *Rp, const SelectBytes *fb, void *scratch,
                                               hipStream_t st) {
  RefineParams R = *Rp;
  DigestParams &D = R.d;
  dig_launch_rank(R, D.totals, st);
  // the cells n_set can name at most, the set full: what the clearing grid is sized from (no memset
  // over cells_cap, which may be far more than the cells in use)
  const uint64_t bound = std::min<uint64_t>(R.cells_cap, (uint64_t)1 << (D.bits + R.sub_bits));
  if (bound) {
    const uint32_t zblk = (uint32_t)std::min<uint64_t>((bound + DIG_DIFF_BLK - 1) / DIG_DIFF_BLK, 4096);
    hipLaunchKernelGGL(dig_zero_kernel, dim3(zblk), dim3(DIG_DIFF_BLK), 0, st, D.cells, R.cells_cap, R.sub_bits, D.totals);
  }
  const uint64_t n = D.sel.src.n, nchunk = (n + SEL_BLK - 1) / SEL_BLK;
  if (!n) return hipGetLastError();
  D.chunks = (uint32_t)std::min<uint64_t>(DIG_CHUNKS, std::max<uint64_t>(1, nchunk / DIG_GRID_MIN));
  const uint64_t nblk = (nchunk + D.chunks - 1) / D.chunks;
  if (const hipError_t e = drp_select_place(&D.sel, fb, scratch, st)) return e;
  hipLaunchKernelGGL(dig_refine_kernel, dim3((uint32_t)nblk), dim3(SEL_BLK), 0, st, R);
  drp_dbg_mark("digest_refine", st);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_select_refined(const RefineParams *Rp, const SelectBytes *fb, void *scratch,
                                                hipStream_t st) {
  RefineParams R = *Rp;
  const uint64_t n = R.d.sel.src.n;
  if (n == 0) return hipMemsetAsync(R.d.sel.n_selected, 0, 8, st);
  if (const hipError_t e = drp_select_place(&R.d.sel, fb, scratch, st)) return e;
  dig_launch_rank(R, nullptr, st);
  hipLaunchKernelGGL(dig_count2_kernel, dim3((uint32_t)((n + SEL_BLK - 1) / SEL_BLK)), dim3(SEL_BLK), 0, st, R);
  const hipError_t e = drp_launch_select_compact(&R.d.sel, st);  // (the last error of all the launches)
  drp_dbg_mark("select_refined", st);
  return e;
}
