// drp_order.hip — gfx950 ordered catch-up: the encoder rows of every segment of a fan-out's output
// (drp_change_src, segment f = rows [row_base[f], row_base[f + 1])) put in ascending `change`
// (unsigned 64-bit, ties by input position), cut to a per-segment limit, and laid end to end again.
// No reference counterpart (the reference has no relay); the field read is `change` of
// messages/schema.proto:1-8.
//
// An LSD radix sort of (change, row) pairs over all segments at once, eight bits per pass, each pass
// stable, then one stable pass on the segment number, then one gather of the ten row columns through
// the permutation. The counts are read on the device: n = row_base[nseg] - row_base[0] rows take part,
// the grids are sized from rows_cap and a workgroup past n leaves on its first load.
//  (0) ord_init: row_base checked (non-decreasing, row_base[nseg] <= rows_cap), n into the control
//      block; an input that fails sorts no rows and keeps none.
//  (1) ord_reduce / ord_plan: the OR and the AND of all keys (per workgroup, then one workgroup over
//      the partial results). A digit in which they agree is the same in every key: its pass moves
//      nothing and is switched off, here on the device. The plan also says where every pass reads:
//      the first one that runs reads the caller's `change` column itself (row = position), the
//      others the pair buffer the pass before them wrote. The segment pass runs only if some digit
//      pass did (the input lies in segment order already) and nseg > 1.
//  (2) per pass, a workgroup of 16 waves over ORD_TILE = 4096 pairs, four per lane (wave w the 64-pair
//      chunks 4w .. 4w + 3, consecutive lanes consecutive pairs):
//      ord_hist: the lanes of a chunk that hold one digit find each other with eight ballots, the
//      first of them adds their number to the workgroup's 256 counts in LDS; counts stored
//      digit-major, hist[digit][workgroup].
//      ord_blocksum / ord_scanbase: a two-level exclusive scan of the flattened table (ORD_SCAN = 1024
//      counts per block; a block's base is the sum of the block sums before it), as drp_fanout.hip's.
//      ord_scatter: the same ballots give a pair's rank among its chunk's pairs of that digit, the
//      chunks' counts per digit (LDS, [chunk][digit]) are scanned over the chunks by one thread per
//      digit, and the pair goes to scanned count + chunk base + rank: stable.
//  (3) ord_cut: one lane per segment: kept = min(count, limit); with DRP_ORDER_KEEP_TIES a cut inside
//      a run of equal keys moves to the run's end (a binary search, the segment is sorted); out_base
//      is the scan of the kept counts.
//  (4) ord_gather: output row j finds its segment in out_base and its source row in the permutation,
//      and copies the ten columns (and sel_idx).
// No global atomics; every loop is bounded; the result is a function of the input alone.
// The digit pass (2) and the gather (4) also serve drp_keyorder.hip, which runs the pass once per
// 8-byte word of a key: drp_launch_order_init / _pass / _gather below are the pieces both chains use,
// and OrderParams::bad / seg_start (null here) are what that chain adds to them.
#include "drp_order.h"

namespace drp {

static_assert(ORD_TILE < 65536, "a chunk base fits the 16-bit counts of ord_scatter");
static_assert(2 * DRP_FANOUT_MAX <= ORD_BINS, "ord_cut: one lane per segment; the segment digit fits a pass");

// (0) the input's validity and its row count
__global__ __launch_bounds__(128) void ord_init_kernel(const OrderParams P) {
  const uint32_t t = threadIdx.x, K = P.nseg;
  bool bad = false;
  if (t < K) bad = P.row_base[t + 1] < P.row_base[t];
  if (t == K) bad = P.row_base[K] > P.rows_cap;
  const int any_bad = __syncthreads_or(bad);
  if (t == 0) {
    OrdCtl &c = *P.ctl;
    const uint64_t b0 = P.row_base[0], n = any_bad ? 0 : P.row_base[K] - b0;
    c.n = n;
    c.b0 = b0;
    c.nwg = (n + ORD_TILE - 1) / ORD_TILE;
    c.valid = !any_bad;
  }
}

// (1a) the OR and the AND of a workgroup's keys
__global__ __launch_bounds__(ORD_BLK) void ord_reduce_kernel(const OrderParams P) {
  __shared__ uint64_t wo[ORD_WAVES], wa[ORD_WAVES];
  const uint64_t n = P.ctl->n, e0 = (uint64_t)blockIdx.x * ORD_TILE;
  if (e0 >= n) return;
  const uint64_t b0 = P.ctl->b0;
  uint64_t o = 0, a = ~0ull;
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    const uint64_t e = e0 + r * ORD_BLK + threadIdx.x;
    if (e < n) {
      const uint64_t k = P.rows.change[b0 + e];
      o |= k;
      a &= k;
    }
  }
  ord_block_or_and(o, a, wo, wa);
  if (threadIdx.x == 0) {
    P.part_or[blockIdx.x] = o;
    P.part_and[blockIdx.x] = a;
  }
}

// (1b) one workgroup: the passes that run and the buffer each one reads (0: the caller's column,
// 1 / 2: a pair buffer; a pass that reads 0 or 2 writes 1, one that reads 1 writes 2)
__global__ __launch_bounds__(ORD_BLK) void ord_plan_kernel(const OrderParams P) {
  __shared__ uint64_t wo[ORD_WAVES], wa[ORD_WAVES];
  OrdCtl &c = *P.ctl;
  const uint64_t n = c.n, nwg = c.nwg;
  uint64_t o = 0, a = ~0ull;
  for (uint64_t k = threadIdx.x; k < nwg; k += ORD_BLK) {
    o |= P.part_or[k];
    a &= P.part_and[k];
  }
  ord_block_or_and(o, a, wo, wa);
  if (threadIdx.x != 0) return;
  const uint64_t diff = n ? o ^ a : 0;  // the bits in which some two keys differ
  uint32_t cur = 0, any = 0;
  for (uint32_t p = 0; p < ORD_PASSES; p++) {
    uint32_t act;
    if (p < ORD_SEG_PASS) act = n != 0 && (!P.skip || ((diff >> (8 * p)) & 0xFFu) != 0);
    else act = any && P.nseg > 1;
    any |= act;
    c.act[p] = act;
    c.src[p] = cur;
    if (act) cur = cur == 1 ? 2 : 1;
  }
  c.final_src = cur;
}

// pair e as pass p reads it and its digit; sb: row_base in LDS (the segment pass)
struct OrdPair {
  uint64_t key;
  uint32_t row;
};
__device__ __forceinline__ OrdPair ord_fetch(const OrderParams &P, uint32_t p, uint32_t src, uint64_t b0, uint64_t e) {
  OrdPair x = {0, 0};
  if (src == 0) {
    x.key = P.rows.change[b0 + e];
    x.row = (uint32_t)(b0 + e);
  } else {
    if (p != ORD_SEG_PASS) x.key = P.key[src - 1][e];  // (the segment pass carries the rows only)
    x.row = P.idx[src - 1][e];
  }
  return x;
}
__device__ __forceinline__ uint32_t ord_digit(const OrderParams &P, uint32_t p, const OrdPair &x, const uint64_t *sb) {
  if (p != ORD_SEG_PASS) return (uint32_t)(x.key >> (8 * p)) & 0xFFu;
  const uint32_t f = ord_seg(sb, P.nseg, x.row);
  return P.bad ? 2 * f + P.bad[x.row] : f;  // (drp_keyorder.hip: the rows left out, behind their segment)
}

// the lanes of the wave that are valid and hold digit d (meaningless for a lane that is not valid)
__device__ __forceinline__ uint64_t ord_peers(bool valid, uint32_t d) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(valid && bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// (2a) the pairs per (digit, workgroup)
__global__ __launch_bounds__(ORD_BLK) void ord_hist_kernel(const OrderParams P, uint32_t p) {
  __shared__ uint32_t h[ORD_BINS];
  __shared__ uint64_t sb[DRP_FANOUT_MAX + 1];
  const OrdCtl &c = *P.ctl;
  if (!c.act[p]) return;
  const uint64_t n = c.n, e0 = (uint64_t)blockIdx.x * ORD_TILE;
  if (e0 >= n) return;
  const uint64_t b0 = c.b0, nwg = c.nwg;
  const uint32_t src = c.src[p], wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  if (threadIdx.x < ORD_BINS) h[threadIdx.x] = 0;
  if (p == ORD_SEG_PASS && threadIdx.x <= P.nseg) sb[threadIdx.x] = P.row_base[threadIdx.x];
  __syncthreads();
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    const uint64_t e = e0 + (wv * ORD_RPL + r) * 64 + lane;
    const bool valid = e < n;
    uint32_t d = 0;
    if (valid) d = ord_digit(P, p, ord_fetch(P, p, src, b0, e), sb);
    const uint64_t m = ord_peers(valid, d);
    if (valid && !(m & below)) atomicAdd(&h[d], (uint32_t)__popcll(m));  // (LDS; one add per digit and chunk)
  }
  __syncthreads();
  if (threadIdx.x < ORD_BINS) P.hist[(uint64_t)threadIdx.x * nwg + blockIdx.x] = h[threadIdx.x];
}

// (2b) the sum of every ORD_SCAN counts of the table's m = 256 * nwg
__global__ __launch_bounds__(ORD_SCAN) void ord_blocksum_kernel(const OrderParams P, uint32_t p) {
  __shared__ uint32_t ws[ORD_SCAN / 64];
  const OrdCtl &c = *P.ctl;
  if (!c.act[p]) return;
  const uint64_t m = (uint64_t)ORD_BINS * c.nwg, g = (uint64_t)blockIdx.x * ORD_SCAN + threadIdx.x;
  if ((uint64_t)blockIdx.x * ORD_SCAN >= m) return;
  uint32_t t;
  (void)block_excl_scan<uint32_t>(g < m ? P.hist[g] : 0, ws, t);
  if (threadIdx.x == 0) P.bsum[blockIdx.x] = t;
}

// (2c) exclusive scan of the table in place: a block's base is the sum of the block sums before it
// (at most blockIdx.x / ORD_SCAN rounds), then a scan within the block. (All sums are <= n < 2^32.)
__global__ __launch_bounds__(ORD_SCAN) void ord_scanbase_kernel(const OrderParams P, uint32_t p) {
  __shared__ uint32_t ws[ORD_SCAN / 64];
  const OrdCtl &c = *P.ctl;
  if (!c.act[p]) return;
  const uint64_t m = (uint64_t)ORD_BINS * c.nwg, g = (uint64_t)blockIdx.x * ORD_SCAN + threadIdx.x;
  if ((uint64_t)blockIdx.x * ORD_SCAN >= m) return;
  uint32_t acc = 0;
  for (uint32_t k = threadIdx.x; k < blockIdx.x; k += ORD_SCAN) acc += P.bsum[k];
  uint32_t base, total;
  (void)block_excl_scan(acc, ws, base);
  const uint32_t v = g < m ? P.hist[g] : 0;
  const uint32_t excl = base + block_excl_scan(v, ws, total);
  if (g < m) P.hist[g] = excl;
}

// (2d) every pair to its place in the pass's output
__global__ __launch_bounds__(ORD_BLK) void ord_scatter_kernel(const OrderParams P, uint32_t p) {
  __shared__ uint16_t cnt[ORD_CHUNKS][ORD_BINS];  // (32 KiB) pairs of a digit in a chunk, then before the chunk
  __shared__ uint32_t gbase[ORD_BINS];
  __shared__ uint64_t sb[DRP_FANOUT_MAX + 1];
  const OrdCtl &c = *P.ctl;
  if (!c.act[p]) return;
  const uint64_t n = c.n, e0 = (uint64_t)blockIdx.x * ORD_TILE;
  if (e0 >= n) return;
  const uint64_t b0 = c.b0, nwg = c.nwg;
  const uint32_t src = c.src[p], dst = src == 1 ? 1 : 0;  // (indices into P.key / P.idx)
  const uint32_t wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  {
    uint32_t *z = reinterpret_cast<uint32_t *>(&cnt[0][0]);
#pragma unroll
    for (uint32_t k = 0; k < ORD_CHUNKS * ORD_BINS / 2 / ORD_BLK; k++) z[k * ORD_BLK + threadIdx.x] = 0;
  }
  if (p == ORD_SEG_PASS && threadIdx.x <= P.nseg) sb[threadIdx.x] = P.row_base[threadIdx.x];
  __syncthreads();
  const uint64_t below = (1ull << lane) - 1ull;
  OrdPair x[ORD_RPL];
  uint32_t d[ORD_RPL], rk[ORD_RPL];
  bool valid[ORD_RPL];
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    const uint32_t ch = wv * ORD_RPL + r;
    const uint64_t e = e0 + ch * 64 + lane;
    valid[r] = e < n;
    d[r] = 0;
    x[r] = OrdPair{0, 0};
    if (valid[r]) {
      x[r] = ord_fetch(P, p, src, b0, e);
      d[r] = ord_digit(P, p, x[r], sb);
    }
    const uint64_t m = ord_peers(valid[r], d[r]);
    rk[r] = (uint32_t)__popcll(m & below);
    if (valid[r] && rk[r] == 0) cnt[ch][d[r]] = (uint16_t)__popcll(m);  // (one writer per chunk and digit)
  }
  __syncthreads();
  if (threadIdx.x < ORD_BINS) {
    uint32_t run = 0;
    for (uint32_t ch = 0; ch < ORD_CHUNKS; ch++) {
      const uint32_t t = cnt[ch][threadIdx.x];
      cnt[ch][threadIdx.x] = (uint16_t)run;  // (run <= ORD_TILE - 1 wherever a pair reads it)
      run += t;
    }
    gbase[threadIdx.x] = P.hist[(uint64_t)threadIdx.x * nwg + blockIdx.x];
  }
  __syncthreads();
  uint64_t *kd = P.key[dst];
  uint32_t *id = P.idx[dst];
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    if (!valid[r]) continue;
    const uint64_t pos = (uint64_t)gbase[d[r]] + cnt[wv * ORD_RPL + r][d[r]] + rk[r];
    if (pos >= n) continue;  // (never: the counts are of these same pairs; n <= rows_cap entries are there)
    if (p != ORD_SEG_PASS) kd[pos] = x[r].key;
    id[pos] = x[r].row;
  }
}

// (3) the rows every segment keeps, and where the outputs start
__global__ __launch_bounds__(64) void ord_cut_kernel(const OrderParams P, const OrdLimits L) {
  const OrdCtl &c = *P.ctl;
  const uint32_t f = threadIdx.x, fs = c.final_src;
  const uint64_t b0 = c.b0;
  uint64_t kept = 0;
  if (f < P.nseg && c.valid) {
    const uint64_t lo = P.row_base[f] - b0, cnt = P.row_base[f + 1] - P.row_base[f];
    kept = umin64(cnt, L.v[f]);
    if ((P.flags & DRP_ORDER_KEEP_TIES) && kept > 0 && kept < cnt) {
      const uint64_t v = P.rows.change[ord_row_at(P, fs, b0, lo + kept - 1)];
      uint64_t a = lo + kept, b = lo + cnt;  // the first position in [a, b) whose key is not v (b: none)
      for (uint32_t k = 0; k < 33 && a < b; k++) {  // (b - a < 2^32)
        const uint64_t mid = a + ((b - a) >> 1);
        if (P.rows.change[ord_row_at(P, fs, b0, mid)] == v) a = mid + 1;
        else b = mid;
      }
      kept = a - lo;
    }
  }
  const uint64_t incl = wave_incl_scan64(kept);
  if (f < P.nseg) P.out_base[f + 1] = incl;
  if (f == 0) P.out_base[0] = 0;
}

// (4) the kept rows' columns, in order
__global__ __launch_bounds__(256) void ord_gather_kernel(const OrderParams P) {
  __shared__ uint64_t ob[DRP_FANOUT_MAX + 1], rb[DRP_FANOUT_MAX + 1];
  const uint32_t K = P.nseg;
  const uint64_t total = P.out_base[K], j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if ((uint64_t)blockIdx.x * 256 >= total) return;
  if (threadIdx.x <= K) {
    ob[threadIdx.x] = P.out_base[threadIdx.x];
    rb[threadIdx.x] = P.row_base[threadIdx.x];
  }
  __syncthreads();
  if (j >= total) return;
  const OrdCtl &c = *P.ctl;
  const uint32_t f = ord_seg(ob, K, j);
  // (< n: start + j - ob[f] < start + kept_f <= the segment's rows)
  const uint64_t s = rb[f] - c.b0 + (P.seg_start ? P.seg_start[f] : 0) + (j - ob[f]);
  const uint64_t i = ord_row_at(P, c.final_src, c.b0, s);
  const drp_change_src &R = P.rows;
  const RowOut &O = P.out;
  O.o_key_off[j] = R.key_off[i];
  O.o_key_len[j] = R.key_len[i];
  O.o_subset_off[j] = R.subset_off[i];
  O.o_subset_len[j] = R.subset_len[i];
  O.o_value_off[j] = R.value_off[i];
  O.o_value_len[j] = R.value_len[i];
  O.o_change[j] = R.change[i];
  O.o_from[j] = R.from[i];
  O.o_to[j] = R.to[i];
  O.o_flags[j] = R.flags[i];
  if (O.sel_idx) O.sel_idx[j] = P.sel_idx[i];
}

}  // namespace drp

using namespace drp;


extern "C" uint64_t drp_order_scratch_bytes(uint64_t rows_cap) { return OrdLayout(rows_cap).end; }

extern "C" void drp_launch_order_init(const OrderParams *P, hipStream_t st) {
  hipLaunchKernelGGL(ord_init_kernel, dim3(1), dim3(128), 0, st, *P);
}

extern "C" void drp_launch_order_pass(const OrderParams *P, uint32_t p, hipStream_t st) {
  const OrdLayout L(P->rows_cap);
  const dim3 tiles((uint32_t)L.nwg), scans((uint32_t)L.nscan);
  hipLaunchKernelGGL(ord_hist_kernel, tiles, dim3(ORD_BLK), 0, st, *P, p);
  hipLaunchKernelGGL(ord_blocksum_kernel, scans, dim3(ORD_SCAN), 0, st, *P, p);
  hipLaunchKernelGGL(ord_scanbase_kernel, scans, dim3(ORD_SCAN), 0, st, *P, p);
  hipLaunchKernelGGL(ord_scatter_kernel, tiles, dim3(ORD_BLK), 0, st, *P, p);
}

// (no output holds more rows than rows_cap, nor more than the limits add up to: out_max)
extern "C" void drp_launch_order_gather(const OrderParams *P, uint64_t out_max, hipStream_t st) {
  const uint64_t most = out_max < P->rows_cap ? out_max : P->rows_cap;
  if (most) hipLaunchKernelGGL(ord_gather_kernel, dim3((uint32_t)((most + 255) / 256)), dim3(256), 0, st, *P);
}

extern "C" hipError_t drp_launch_order(const OrderParams *Pp, const OrdLimits *lim, uint64_t out_max, void *scratch,
                                       hipStream_t st) {
  OrderParams P = *Pp;
  const OrdLayout L(P.rows_cap);
  L.place(P, scratch);
  drp_launch_order_init(&P, st);
  hipLaunchKernelGGL(ord_reduce_kernel, dim3((uint32_t)L.nwg), dim3(ORD_BLK), 0, st, P);
  hipLaunchKernelGGL(ord_plan_kernel, dim3(1), dim3(ORD_BLK), 0, st, P);
  for (uint32_t p = 0; p < ORD_PASSES; p++) {
    if (p == ORD_SEG_PASS && P.nseg == 1) break;
    drp_launch_order_pass(&P, p, st);
  }
  drp_dbg_mark("order_sort", st);
  hipLaunchKernelGGL(ord_cut_kernel, dim3(1), dim3(64), 0, st, P, *lim);
  drp_launch_order_gather(&P, out_max, st);
  drp_dbg_mark("order_gather", st);
  return hipGetLastError();
}
