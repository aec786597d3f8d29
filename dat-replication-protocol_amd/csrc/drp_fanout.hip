// drp_fanout.hip — gfx950 fan-out of decoded Changes: up to DRP_FANOUT_MAX filters (drp_filter)
// over one pass of the Change columns, the rows each filter keeps compacted stably into encoder
// rows (drp_change_src), the outputs end to end in filter order, and a splice table that says where
// the blob frames belong in each output. No reference counterpart (the reference has no relay);
// the order the splice table restores is the one encode.js:77-100 keeps (a Change waits for the
// blob before it), the fields the predicates read are those of messages/schema.proto:1-8.
//
// The steps of drp_select.hip (ballot, scan, scatter), reshaped so that nothing per row is repeated
// per filter. A workgroup of 16 waves takes FAN_ROWS = 4096 rows, four per lane (wave w the 64-row
// chunks 4w .. 4w + 3, consecutive lanes consecutive rows):
//  (1) fan_count: every row's columns are loaded once into registers (only the columns some filter
//      names); the filters are walked wave-uniformly from a table in LDS, one ballot per (filter,
//      chunk) stored filter-major, mask[f][i >> 6]; one count per (filter, workgroup). The blob rows
//      are one more plane, mask[K]: the splice table needs their ballots and counts.
//  (2) fan_blocksum / fan_scanbase: a two-level exclusive scan of the flattened counts [f][workgroup]
//      (FAN_SCAN = 1024 counts per block; a block's base is the sum of the block sums before it).
//      row_base[f] is the scanned value at [f][0].
//  (3) fan_scatter: per workgroup every filter's 64 ballot words and the scan of their popcounts go
//      to LDS (one wave per filter, one word per lane); a row kept by at least one filter loads its
//      source columns once and stores them to its slot in every output that keeps it.
//  (4) fan_splice: blob j's row and, per filter, the rows of that output before it, from the same
//      ballot words and scanned counts (no predicate is evaluated again).
// No global atomics (same-address atomics serialise across the 8 XCDs); every loop is bounded.
#include "drp_select.h"  // (pred_load / pred_conds, row_load / row_store)

namespace drp {

// (FAN_BLK, FAN_WAVES, FAN_RPL, FAN_ROWS, FAN_CHUNKS: drp_select.h)
constexpr uint32_t FAN_SCAN = 1024;                                            // counts per first-level scan block
constexpr uint32_t FAN_PLANES = DRP_FANOUT_MAX + 1;                            // the filters and the blob rows
static_assert(FAN_CHUNKS == 64, "fan_prefix scans one ballot word per lane");

// (1) the ballot word of every (filter, 64 rows) and the rows kept per (filter, workgroup)
__global__ __launch_bounds__(FAN_BLK) void fan_count_kernel(const FanParams P) {
  __shared__ RowFilter sf[DRP_FANOUT_MAX];
  __shared__ uint32_t wcnt[FAN_PLANES][FAN_WAVES];
  const RowSrc &S = P.src;
  const uint32_t K = P.nfilters, wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  if (threadIdx.x < K * (sizeof(RowFilter) / 4))  // (K * 8 <= 512 words)
    reinterpret_cast<uint32_t *>(sf)[threadIdx.x] = reinterpret_cast<const uint32_t *>(P.filt)[threadIdx.x];
  const uint64_t word0 = (uint64_t)blockIdx.x * FAN_CHUNKS + wv * FAN_RPL;  // (< nwords: the grid is nwg)
  PredRow row[FAN_RPL];
  bool ok[FAN_RPL], blob[FAN_RPL];
#pragma unroll
  for (uint32_t r = 0; r < FAN_RPL; r++) {
    const uint64_t i = (word0 + r) * 64 + lane;
    ok[r] = blob[r] = false;
    row[r] = PredRow{0, 0, 0, 0, 0, 0};
    if (i < S.n) {
      const uint32_t ty = S.type[i] & 0x3Fu;
      blob[r] = ty == DRP_TYPE_BLOB;
      if (ty == DRP_TYPE_CHANGE) {
        row[r].flags = S.cols.flags[i];
        ok[r] = !(row[r].flags & DRP_F_BAD);
      }
    }
    if (ok[r]) pred_load(S, i, P.any_flags, P.any_bytes, row[r]);
  }
  __syncthreads();
  for (uint32_t f = 0; f < K; f++) {  // (wave-uniform: K is a launch argument)
    const RowFilter F = sf[f];
    const uint8_t *fb = P.fbytes + (size_t)f * FAN_FBYTES;
    uint64_t *mrow = P.mask + (uint64_t)f * P.nwords + word0;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < FAN_RPL; r++) {
      const bool keep = ok[r] && pred_conds(S, F, fb, fb + DRP_SEL_MAX_BYTES, row[r]);
      const uint64_t b = __ballot(keep);
      if (lane == 0) mrow[r] = b;
      cnt += (uint32_t)__popcll(b);
    }
    if (lane == 0) wcnt[f][wv] = cnt;
  }
  {
    uint64_t *mrow = P.mask + (uint64_t)K * P.nwords + word0;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < FAN_RPL; r++) {
      const uint64_t b = __ballot(blob[r]);
      if (lane == 0) mrow[r] = b;
      cnt += (uint32_t)__popcll(b);
    }
    if (lane == 0) wcnt[K][wv] = cnt;
  }
  __syncthreads();
  if (threadIdx.x <= K) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < FAN_WAVES; k++) s += wcnt[threadIdx.x][k];
    P.block_cnt[(uint64_t)threadIdx.x * P.nwg + blockIdx.x] = s;
  }
}

// (2a) the sum of every FAN_SCAN counts
__global__ __launch_bounds__(FAN_SCAN) void fan_blocksum_kernel(const uint64_t *cnt, uint64_t m, uint64_t *bsum) {
  __shared__ uint64_t sw[FAN_SCAN / WAVE];
  const uint64_t g = (uint64_t)blockIdx.x * FAN_SCAN + threadIdx.x;
  uint64_t t;
  (void)block_excl_scan<uint64_t>(g < m ? cnt[g] : 0, sw, t);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}

// (2b) exclusive scan of the m = (K + 1) * nwg counts in place: a block's base is the sum of the
// block sums before it (at most blockIdx.x / FAN_SCAN rounds), then a scan within the block. The
// value at [f][0] is row_base[f]; the total past the last count (rows and blob rows) is *gtotal.
__global__ __launch_bounds__(FAN_SCAN) void fan_scanbase_kernel(const FanParams P, uint64_t m) {
  __shared__ uint64_t sw[FAN_SCAN / WAVE];
  uint64_t acc = 0;
  for (uint32_t k = threadIdx.x; k < blockIdx.x; k += FAN_SCAN) acc += P.bsum[k];
  uint64_t base, total;
  (void)block_excl_scan(acc, sw, base);
  const uint64_t g = (uint64_t)blockIdx.x * FAN_SCAN + threadIdx.x;
  const uint64_t v = g < m ? P.block_cnt[g] : 0;
  const uint64_t excl = base + block_excl_scan(v, sw, total);
  if (g < m) {
    P.block_cnt[g] = excl;
    if (g % P.nwg == 0) {
      const uint64_t f = g / P.nwg;
      if (f <= P.nfilters) P.row_base[f] = excl;
    }
    if (g == m - 1) *P.gtotal = excl + v;
  }
}

// per workgroup and plane f < planes: words[f][c] = the plane's ballot word of the workgroup's chunk
// c, pre[f][c] = the bits of the words before c, base[f] = the plane's scanned count of the workgroup
__device__ __forceinline__ void fan_prefix(const FanParams &P, uint32_t planes, uint64_t (*words)[FAN_CHUNKS],
                                           uint32_t (*pre)[FAN_CHUNKS], uint64_t *base) {
  const uint32_t wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  for (uint32_t f = wv; f < planes; f += FAN_WAVES) {
    const uint64_t w = P.mask[(uint64_t)f * P.nwords + (uint64_t)blockIdx.x * FAN_CHUNKS + lane];
    const uint32_t cnt = (uint32_t)__popcll(w);
    words[f][lane] = w;
    pre[f][lane] = wave_incl_scan32(cnt) - cnt;
    if (lane == 0) base[f] = P.block_cnt[(uint64_t)f * P.nwg + blockIdx.x];
  }
  __syncthreads();
}

// (3) every kept row's columns to its slot in every output that keeps it
__global__ __launch_bounds__(FAN_BLK) void fan_scatter_kernel(const FanParams P) {
  __shared__ uint64_t words[DRP_FANOUT_MAX][FAN_CHUNKS];  // (32 KiB: read 2 K times per chunk below)
  __shared__ uint32_t pre[DRP_FANOUT_MAX][FAN_CHUNKS];
  __shared__ uint64_t base[DRP_FANOUT_MAX];
  const uint32_t K = P.nfilters;
  if (P.row_base[K] > P.rows_cap) return;  // (uniform over the grid: nothing is written)
  fan_prefix(P, K, words, pre, base);
  const uint32_t wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll 1
  for (uint32_t r = 0; r < FAN_RPL; r++) {
    const uint32_t ch = wv * FAN_RPL + r;
    uint64_t any = 0;
    for (uint32_t f = 0; f < K; f++) any |= words[f][ch];  // (wave-uniform LDS reads)
    if (!((any >> lane) & 1ull)) continue;  // (kept by no filter; a bit is only ever set for a row < n)
    const uint64_t i = ((uint64_t)blockIdx.x * FAN_CHUNKS + ch) * 64 + lane;
    const EncRow row = row_load(P.src, i);
    for (uint32_t f = 0; f < K; f++) {
      const uint64_t b = words[f][ch];
      if (!((b >> lane) & 1ull)) continue;
      const uint64_t slot = base[f] + pre[f][ch] + (uint32_t)__popcll(b & below);  // (< row_base[K] <= rows_cap)
      row_store(P.out, slot, row, i);
    }
  }
}

// (4) the splice table: blob j's source row, and for every filter the rows of its output before it
__global__ __launch_bounds__(FAN_BLK) void fan_splice_kernel(const FanParams P) {
  __shared__ uint64_t words[FAN_PLANES][FAN_CHUNKS];
  __shared__ uint32_t pre[FAN_PLANES][FAN_CHUNKS];
  __shared__ uint64_t base[FAN_PLANES];
  const uint32_t K = P.nfilters;
  const uint64_t first = P.row_base[K], nb = *P.gtotal - first;  // (the blob plane's counts follow the filters')
  if (blockIdx.x == 0 && threadIdx.x == 0) *P.n_blobs = nb;
  if (nb > P.blob_cap) return;  // (uniform over the grid: the arrays are not written)
  fan_prefix(P, K + 1, words, pre, base);
  const uint32_t wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll 1
  for (uint32_t r = 0; r < FAN_RPL; r++) {
    const uint32_t ch = wv * FAN_RPL + r;
    const uint64_t bw = words[K][ch];
    if (!((bw >> lane) & 1ull)) continue;
    const uint64_t j = base[K] - first + pre[K][ch] + (uint32_t)__popcll(bw & below);  // (< nb <= blob_cap)
    P.blob_row[j] = ((uint64_t)blockIdx.x * FAN_CHUNKS + ch) * 64 + lane + P.row_bias;
    for (uint32_t f = 0; f < K; f++) {
      const uint64_t b = words[f][ch];
      P.blob_rank[(uint64_t)f * P.blob_cap + j] = base[f] - P.row_base[f] + pre[f][ch] + (uint32_t)__popcll(b & below);
    }
  }
}

// after the encode: where every output starts in the encoded bytes, and every blob's byte position
// within every output
__global__ __launch_bounds__(256) void fan_gather_kernel(const uint64_t *frame_off, const uint64_t *row_base,
                                                         uint32_t K, const uint64_t *rank, uint64_t nb,
                                                         uint64_t *out_off, uint64_t *blob_pos) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t <= K) out_off[t] = frame_off[row_base[t]];
  if (t < (uint64_t)K * nb) {
    const uint64_t rb = row_base[t / nb];
    blob_pos[t] = frame_off[rb + rank[t]] - frame_off[rb];
  }
}

}  // namespace drp

using namespace drp;

static uint64_t fan_nwg(uint64_t n) { return (n + FAN_ROWS - 1) / FAN_ROWS; }

namespace {
struct FanLayout {
  uint64_t filt, fbytes, mask, cnt, bsum, tot, end;
  FanLayout(uint64_t n, uint32_t K) {
    const uint64_t nwg = fan_nwg(n), planes = (uint64_t)K + 1, m = planes * nwg;
    filt = 0;
    fbytes = al((uint64_t)K * sizeof(RowFilter));
    mask = fbytes + (uint64_t)K * FAN_FBYTES;
    cnt = mask + al(planes * nwg * FAN_CHUNKS * 8);
    bsum = cnt + al(m * 8);
    tot = bsum + al(((m + FAN_SCAN - 1) / FAN_SCAN) * 8);
    end = tot + 256;
  }
};
}  // namespace

extern "C" uint64_t drp_fanout_scratch_bytes(uint64_t n, uint32_t nfilters) { return FanLayout(n, nfilters).end; }

extern "C" void drp_fanout_place(FanParams *P, void *scratch) {
  const FanLayout L(P->src.n, P->nfilters);
  uint8_t *sc = static_cast<uint8_t *>(scratch);
  P->filt = reinterpret_cast<const RowFilter *>(sc + L.filt);
  P->fbytes = sc + L.fbytes;
  P->mask = reinterpret_cast<uint64_t *>(sc + L.mask);
  P->block_cnt = reinterpret_cast<uint64_t *>(sc + L.cnt);
  P->bsum = reinterpret_cast<uint64_t *>(sc + L.bsum);
  P->gtotal = reinterpret_cast<uint64_t *>(sc + L.tot);
  P->nwg = fan_nwg(P->src.n);
  P->nwords = P->nwg * FAN_CHUNKS;
}

extern "C" hipError_t drp_launch_fanout_ballot(const FanParams *Pp, hipStream_t st) {
  const FanParams &P = *Pp;
  if (P.src.n == 0) return hipSuccess;
  if (P.nwg >= (1ull << 31) / FAN_PLANES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fan_count_kernel, dim3((uint32_t)P.nwg), dim3(FAN_BLK), 0, st, P);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_fanout_scan(const FanParams *Pp, hipStream_t st) {
  const FanParams &P = *Pp;
  if (P.src.n == 0) {  // no rows: every output and the blob list are empty
    hipError_t e = hipMemsetAsync(P.row_base, 0, ((size_t)P.nfilters + 1) * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(P.gtotal, 0, 8, st);
    return e;
  }
  const uint64_t m = ((uint64_t)P.nfilters + 1) * P.nwg, nb = (m + FAN_SCAN - 1) / FAN_SCAN;
  hipLaunchKernelGGL(fan_blocksum_kernel, dim3((uint32_t)nb), dim3(FAN_SCAN), 0, st, P.block_cnt, m, P.bsum);
  hipLaunchKernelGGL(fan_scanbase_kernel, dim3((uint32_t)nb), dim3(FAN_SCAN), 0, st, P, m);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_fanout_count(const FanParams *Pp, hipStream_t st) {
  if (const hipError_t e = drp_launch_fanout_ballot(Pp, st)) return e;
  const hipError_t e = drp_launch_fanout_scan(Pp, st);
  if (Pp->src.n) drp_dbg_mark("fanout_count", st);
  return e;
}

extern "C" hipError_t drp_launch_fanout_scatter(const FanParams *Pp, hipStream_t st) {
  if (Pp->src.n == 0) return hipSuccess;
  hipLaunchKernelGGL(fan_scatter_kernel, dim3((uint32_t)Pp->nwg), dim3(FAN_BLK), 0, st, *Pp);
  drp_dbg_mark("fanout_scatter", st);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_fanout_splice(const FanParams *Pp, hipStream_t st) {
  if (Pp->src.n == 0) return hipMemsetAsync(Pp->n_blobs, 0, 8, st);
  hipLaunchKernelGGL(fan_splice_kernel, dim3((uint32_t)Pp->nwg), dim3(FAN_BLK), 0, st, *Pp);
  drp_dbg_mark("fanout_splice", st);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_fanout_gather(const uint64_t *frame_off, const uint64_t *row_base, uint32_t nfilters,
                                               const uint64_t *rank, uint64_t nb, uint64_t *out_off, uint64_t *blob_pos,
                                               hipStream_t st) {
  const uint64_t work = (uint64_t)nfilters * nb > nfilters ? (uint64_t)nfilters * nb : (uint64_t)nfilters + 1;
  if ((work + 255) / 256 >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fan_gather_kernel, dim3((uint32_t)((work + 255) / 256)), dim3(256), 0, st, frame_off, row_base,
                     nfilters, rank, nb, out_off, blob_pos);
  return hipGetLastError();
}
