// drp_select.hip — gfx950 select of decoded Changes: a predicate over the Change columns and a
// stable compaction of the rows it keeps into encoder rows (drp_change_src, offsets absolute into
// the wire), so the encoder (drp_encode.hip) re-encodes them with the received wire as its heap.
// No reference counterpart: the reference has no relay; the fields the predicate reads are those
// of messages/schema.proto:1-8 (subset, key, change).
//
// The same three steps as enc_size / enc_blocksum / enc_addbase: (1) one row per lane, the
// predicate's wave ballot kept as one word per 64 rows and its popcounts summed across the
// workgroup's waves in LDS into one count per workgroup, (2) one workgroup scans the counts,
// (3) every selected row finds its slot from its workgroup's base, the popcounts of the waves
// before it and the ballot bits below its lane, and writes its columns there. No global atomics;
// the order of the rows is kept. The columns are read one 1 / 4 / 8-byte element per lane,
// consecutive lanes consecutive elements; step (1) reads only the columns the filter names and
// step (3) only the rows kept (the byte compares read wire bytes only of rows whose lengths match).
#include "drp_select.h"  // (sel_pred, sel_publish, row_load / row_store, SEL_BLK)

namespace drp {

constexpr uint32_t SEL_KNOWN = DRP_SEL_CHANGE_RANGE | DRP_SEL_SUBSET_EQ | DRP_SEL_SUBSET_NONE | DRP_SEL_KEY_PREFIX;

// the filter's byte strings into device memory (they travel as launch arguments: no host buffer
// to keep alive behind an asynchronous copy)
__global__ __launch_bounds__(2 * DRP_SEL_MAX_BYTES) void sel_filter_kernel(const SelectBytes F, uint8_t *dst) {
  dst[threadIdx.x] = F.b[threadIdx.x];
}

// (1) the ballot word of every 64 rows and the rows kept per workgroup
__global__ __launch_bounds__(SEL_BLK) void sel_count_kernel(const SelectParams P) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  sel_publish(P, i < P.src.n && sel_pred(P, i));
}

// (2) exclusive scan of the workgroup counts in place (any number of them: SEL_BLK per round with
// a running carry); the total is the number of rows kept
__global__ __launch_bounds__(SEL_BLK) void sel_scan_kernel(const SelectParams P, uint64_t nblk) {
  __shared__ uint64_t part[SEL_WAVES];
  const uint64_t total = block_scan_rounds(
      nblk, part, [&](uint64_t b) { return P.block_cnt[b]; }, [&](uint64_t b, uint64_t ex) { P.block_cnt[b] = ex; });
  if (threadIdx.x == 0) *P.n_selected = total;
}

// (3) every kept row's columns to its slot
__global__ __launch_bounds__(SEL_BLK) void sel_scatter_kernel(const SelectParams P) {
  __shared__ uint32_t wcnt[SEL_WAVES];
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t b = P.mask[i >> 6];  // (wave-uniform; written by sel_count_kernel for every wave of the grid)
  if (lane == 0) wcnt[wv] = (uint32_t)__popcll(b);
  __syncthreads();
  if (!((b >> lane) & 1ull)) return;
  uint64_t slot = P.block_cnt[blockIdx.x];
  for (uint32_t k = 0; k < wv; k++) slot += wcnt[k];
  slot += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  row_store(P.out, slot, row_load(P.src, i), i);
}

}  // namespace drp

using namespace drp;

extern "C" uint32_t drp_select_known_flags(void) { return SEL_KNOWN; }

// scratch: the filter's byte strings, the ballot words (one per 64 rows, for whole workgroups),
// the workgroup counts
static uint64_t sel_nblk(uint64_t n) { return (n + SEL_BLK - 1) / SEL_BLK; }
static uint64_t sel_mask_bytes(uint64_t n) { return al(sel_nblk(n) * SEL_WAVES * 8); }
extern "C" uint64_t drp_select_scratch_bytes(uint64_t n) {
  return 2 * DRP_SEL_MAX_BYTES + sel_mask_bytes(n) + sel_nblk(n) * 8 + 256;
}

// P's scratch pointers into `scratch` and the filter's byte strings onto the device (n > 0)
extern "C" hipError_t drp_select_place(SelectParams *P, const SelectBytes *fb, void *scratch, hipStream_t st) {
  if (sel_nblk(P->src.n) >= (1ull << 31)) return hipErrorInvalidValue;
  uint8_t *sc = static_cast<uint8_t *>(scratch);
  P->subset = sc;
  P->prefix = sc + DRP_SEL_MAX_BYTES;
  P->mask = reinterpret_cast<uint64_t *>(sc + 2 * DRP_SEL_MAX_BYTES);
  P->block_cnt = reinterpret_cast<uint64_t *>(sc + 2 * DRP_SEL_MAX_BYTES + sel_mask_bytes(P->src.n));
  if (P->f.flags & (DRP_SEL_SUBSET_EQ | DRP_SEL_KEY_PREFIX))
    hipLaunchKernelGGL(sel_filter_kernel, dim3(1), dim3(2 * DRP_SEL_MAX_BYTES), 0, st, *fb, sc);
  return hipSuccess;
}

// steps (2) and (3) over the ballot words and workgroup counts a step (1) has left in P's scratch
extern "C" hipError_t drp_launch_select_compact(const SelectParams *Pp, hipStream_t st) {
  const SelectParams &P = *Pp;
  const uint64_t nblk = sel_nblk(P.src.n);
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(SEL_BLK), 0, st, P, nblk);
  hipLaunchKernelGGL(sel_scatter_kernel, dim3((uint32_t)nblk), dim3(SEL_BLK), 0, st, P);
  return hipGetLastError();
}

// step (2) alone, for drp_store.hip: cnt[0, nblk) scanned in place (exclusive), *total = their sum
extern "C" hipError_t drp_launch_count_scan(uint64_t *cnt, uint64_t nblk, uint64_t *total, hipStream_t st) {
  SelectParams P = {};
  P.block_cnt = cnt;
  P.n_selected = total;
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(SEL_BLK), 0, st, P, nblk);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_select(const SelectParams *Pp, const SelectBytes *fb, void *scratch, hipStream_t st) {
  SelectParams P = *Pp;
  if (P.src.n == 0) return hipMemsetAsync(P.n_selected, 0, 8, st);
  if (const hipError_t e = drp_select_place(&P, fb, scratch, st)) return e;
  hipLaunchKernelGGL(sel_count_kernel, dim3((uint32_t)sel_nblk(P.src.n)), dim3(SEL_BLK), 0, st, P);
  const hipError_t e = drp_launch_select_compact(&P, st);  // (the last error of all the launches)
  drp_dbg_mark("select", st);
  return e;
}
