// drp_latest.hip — gfx950 latest-per-key compaction of decoded Changes: of the rows the select
// predicate keeps (drp_select.h), for every identity (subset presence, subset bytes, key bytes) the
// one row with the greatest `change`, the later row on a tie, written as drp_select.hip writes its
// rows (a stable compaction into encoder rows whose offsets are absolute into the wire).
// No reference counterpart: the reference has no relay; the fields read are subset, key and change
// of messages/schema.proto:1-8.
//
// The grouping is an insert-only open-addressing table over the rows' byte strings, probed
// linearly, at most half full. Whatever one workgroup writes and another reads within one kernel
// goes through an agent-scope atomic and nothing else does, which the split into kernels ensures:
//   lat_insert  one row per lane: the predicate, the identity's hash (XXH64 of the key, the subset's
//               merged in), then along the probe sequence at most one compare-and-swap per slot of
//               the slot's rep word from 0 to hash tag | row + 1 (none where an atomic load finds
//               the word set: it is written once). A swap that took place claims the slot for the
//               row's group; otherwise the word it returned, or the load, names the row that did,
//               and that row's identity (the tag, then its decoded columns and wire bytes: kernel
//               inputs, plain reads) says whether this is the group's slot or the probe moves on.
//               No lane waits for another; the loop ends after nslots steps at the latest. Then an
//               atomic max of the row's change into the slot's second word (skipped where an atomic
//               load already shows as much: the word only grows), and the slot number into
//               slot[row] (a plain store that only the same row's lane of the next kernels reads).
//               Such a load may be served by a stale line of the XCD's L2: the words only move
//               from 0 to set, or up, so a stale value is never wrong, it only costs the atomic.
//   lat_pick    a row whose change equals its slot's maximum: an atomic max of row + 1 into the
//               slot's third word (the maxima are complete: a kernel boundary lies in between).
//   lat_keep    a row is kept iff that word names it; the ballot words and workgroup counts in the
//               form sel_count_kernel leaves them, for the select's scan and scatter.
// Which row claimed a slot and where a group landed decide nothing: every group's two maxima are
// over the same rows whatever the order, and the kept rows leave in row order.
//
// The same for every filter of a fan-out (drp_fanout_latest_*): fan_count (drp_fanout.hip) has left
// one ballot plane per filter; the grouping is done once, the reduction per filter, under the rule
// above (the rep words and the state words through agent-scope atomics, the rest across kernel
// boundaries):
//   flat_group  lat_insert's probe (lat_group, one function, two callers) for every row that some
//               plane keeps, over a table of rep words only; the row's slot, and per 64 rows the
//               ballot of the rows whose swap claimed a slot: one row per group.
//   flat_scan / flat_number   the groups numbered densely: a group's number is the rank of the row
//               that claimed its slot among the rows that claimed one (a scan of the ballots; rep
//               names the row); group[row] instead of the slot. The numbers depend on which rows
//               won their swaps; nothing in the result does.
//   flat_max / flat_pick / flat_keep   per pass of up to `pass` filters, over state words
//               [group][filter of the pass][2] cleared before the pass: lat_insert's maximum, lat_pick
//               and lat_keep for every filter of the pass per row, each behind the row's bit in the
//               filter's plane; flat_keep overwrites the pass's planes and workgroup counts in the
//               form fan_count left them, for the fan-out's scan and scatter.
#include "drp_select.h"

namespace drp {

// word w of slot s (W words per slot)
template <uint32_t W>
__device__ __forceinline__ uint64_t *lat_word(const LatTable &T, uint64_t s, uint32_t w) { return T.tab + W * s + w; }

// wire bytes [a, a + len) == [b, b + len) (both ranges inside the wire)
__device__ __forceinline__ bool lat_bytes_eq(const RowSrc &P, uint64_t a, uint64_t b, uint32_t len) {
  return bytes_eq(P.bytes + a, P.bytes + b, len);  // (drp_select.h; drp_store.hip compares with it too)
}

// candidate row j (it claimed a slot: its ranges are inside the wire) has this identity
__device__ __forceinline__ bool lat_same(const RowSrc &P, uint64_t j, bool has, uint64_t koff, uint32_t klen,
                                         uint64_t soff, uint32_t slen) {
  const drp_changes &c = P.cols;
  if (((c.flags[j] & DRP_F_SUBSET) != 0) != has || c.key_len[j] != klen) return false;
  if (has && c.subset_len[j] != slen) return false;
  const uint64_t base = P.payload_off[j] + row_shift(P, j);
  if (!lat_bytes_eq(P, base + c.key_off[j], koff, klen)) return false;
  return !has || lat_bytes_eq(P, base + c.subset_off[j], soff, slen);
}

// The slot of row i's group (i: a well-formed Change that some predicate keeps), claimed by this row
// or by an earlier visitor of the same identity; LAT_NONE for a row whose key or subset range leaves
// the wire: it is never read and is no candidate. W: the table's words per slot. claimed: this row's
// swap took the slot (one row per group sees that).
template <uint32_t W>
__device__ __forceinline__ uint64_t lat_group(const RowSrc &P, const LatTable &T, uint64_t i, bool &claimed) {
  claimed = false;
  const drp_changes &c = P.cols;
  const bool has = (c.flags[i] & DRP_F_SUBSET) != 0;
  const uint64_t base = P.payload_off[i] + row_shift(P, i);
  const uint64_t koff = base + c.key_off[i], soff = base + c.subset_off[i];
  const uint32_t klen = c.key_len[i], slen = has ? c.subset_len[i] : 0;
  if (!wire_has(P, koff, klen) || (has && !wire_has(P, soff, slen))) return LAT_NONE;
  uint64_t h = xxh::xxh64(P.bytes + koff, klen);
  if (has) h = xxh::merge(h, xxh::xxh64(P.bytes + soff, slen));  // (an empty subset still changes h)
  h &= T.hash_mask;
  const uint64_t smask = T.nslots - 1, word = (h & T.tag_mask) | (i + 1);
  uint64_t s = h & smask;
  for (uint64_t step = 0; step < T.nslots; step++, s = (s + 1) & smask) {
    // rep is written once, so an atomic load that finds it set saves the swap (a stale 0 only
    // costs the swap, which leaves the word it found in `seen`)
    uint64_t seen = ld_agent(lat_word<W>(T, s, 0));
    if (seen == 0 && __hip_atomic_compare_exchange_strong(lat_word<W>(T, s, 0), &seen, word, __ATOMIC_RELAXED,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      claimed = true;
      return s;
    }
    if (((seen ^ word) & T.tag_mask) == 0 && lat_same(P, (seen & ~T.tag_mask) - 1, has, koff, klen, soff, slen))
      return s;
  }
  return LAT_NONE;  // (not reached: the table is at most half full)
}

// an atomic max of v into *p. The word only grows: a load that already shows v or more saves the
// atomic (a stale, smaller value only costs it), which is what keeps a hot key's rows off one address
__device__ __forceinline__ void lat_max(uint64_t *p, uint64_t v) {
  if (ld_agent(p) < v) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(SEL_BLK) void lat_insert_kernel(const LatestParams L) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  if (i >= L.sel.src.n) return;
  uint64_t mine = LAT_NONE;
  if (sel_pred(L.sel, i)) {
    bool claimed;
    mine = lat_group<3>(L.sel.src, L.t, i, claimed);
    if (mine != LAT_NONE) lat_max(lat_word<3>(L.t, mine, 1), L.sel.src.cols.change[i]);
  }
  L.slot[i] = mine;
}

__global__ __launch_bounds__(SEL_BLK) void lat_pick_kernel(const LatestParams L) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  if (i >= L.sel.src.n) return;
  const uint64_t s = L.slot[i];
  if (s == LAT_NONE) return;
  // (a group whose only change is 0 matches the cleared word)
  if (L.sel.src.cols.change[i] == *lat_word<3>(L.t, s, 1)) lat_max(lat_word<3>(L.t, s, 2), i + 1);
}

// sel_count_kernel with the predicate "the row its group picked"
__global__ __launch_bounds__(SEL_BLK) void lat_keep_kernel(const LatestParams L) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  bool keep = false;
  if (i < L.sel.src.n) {
    const uint64_t s = L.slot[i];
    keep = s != LAT_NONE && *lat_word<3>(L.t, s, 2) == i + 1;
  }
  sel_publish(L.sel, keep);
}

// ---- latest per key under every filter of a fan-out -------------------------------------------
// fan_count has left one ballot plane per filter, mask[f][row >> 6]. A row's wave reads a plane's
// word of its 64 rows wave-uniformly; row i is in plane f iff bit i & 63 of that word is set (a bit
// is only ever set for a well-formed Change below n).
__device__ __forceinline__ uint64_t flat_plane(const FanParams &F, uint32_t f, uint64_t w) {
  return F.mask[(uint64_t)f * F.nwords + w];
}
// the two words of (group g, filter k of the pass)
__device__ __forceinline__ uint64_t *flat_state(const FanLatestParams &L, uint64_t g, uint32_t k) {
  return L.state + (g * L.nf + k) * 2;
}

// the grouping, once for all filters: lat_insert's probe for every row that some plane keeps; the
// row's slot, and per 64 rows the ballot of the rows that claimed theirs (one per group)
__global__ __launch_bounds__(SEL_BLK) void flat_group_kernel(const FanLatestParams L) {
  const FanParams &F = L.fan;
  const uint64_t w = (uint64_t)blockIdx.x * SEL_WAVES + uniform32(threadIdx.x >> 6);
  const uint64_t i = w * 64 + lane_id();
  if (i >= F.src.n) return;
  uint64_t any = 0;
  for (uint32_t f = 0; f < F.nfilters; f++) any |= flat_plane(F, f, w);
  bool claimed = false;
  L.group[i] = ((any >> lane_id()) & 1ull) ? lat_group<1>(F.src, L.t, i, claimed) : LAT_NONE;
  const uint64_t b = __ballot(claimed);
  if (lane_id() == 0) L.lead[w] = b;
}

// exclusive scan of the m claim ballots' popcounts, one workgroup: every thread sums a run of
// consecutive words, the runs' sums are scanned across the workgroup, every thread writes its run
__global__ __launch_bounds__(SEL_BLK) void flat_scan_kernel(const FanLatestParams L, uint64_t m) {
  __shared__ uint64_t part[SEL_WAVES];
  const uint64_t per = (m + SEL_BLK - 1) / SEL_BLK, a = umin64(m, threadIdx.x * per), b = umin64(m, a + per);
  uint64_t s = 0;
  for (uint64_t g = a; g < b; g++) s += (uint64_t)__popcll(L.lead[g]);
  uint64_t total;
  uint64_t run = block_excl_scan(s, part, total);
  for (uint64_t g = a; g < b; g++) {
    L.lead_base[g] = run;
    run += (uint64_t)__popcll(L.lead[g]);
  }
}

// group[row]: from the slot to the group's number, the rank of the row that claimed the slot among
// the rows that claimed one (rep names that row; complete: a kernel boundary lies in between)
__global__ __launch_bounds__(SEL_BLK) void flat_number_kernel(const FanLatestParams L) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  if (i >= L.fan.src.n) return;
  const uint64_t s = L.group[i];
  if (s == LAT_NONE) return;
  const uint64_t r = (*lat_word<1>(L.t, s, 0) & ~L.t.tag_mask) - 1;
  L.group[i] = L.lead_base[r >> 6] + (uint64_t)__popcll(L.lead[r >> 6] & ((1ull << (r & 63)) - 1ull));
}

// per pass, every filter of the pass per row: the greatest change the filter keeps in the row's group
__global__ __launch_bounds__(SEL_BLK) void flat_max_kernel(const FanLatestParams L) {
  const FanParams &F = L.fan;
  const uint64_t w = (uint64_t)blockIdx.x * SEL_WAVES + uniform32(threadIdx.x >> 6);
  const uint64_t i = w * 64 + lane_id();
  if (i >= F.src.n) return;
  const uint64_t s = L.group[i];
  if (s == LAT_NONE) return;
  const uint64_t ch = F.src.cols.change[i];
  for (uint32_t k = 0; k < L.nf; k++)
    if ((flat_plane(F, L.f0 + k, w) >> lane_id()) & 1ull) lat_max(flat_state(L, s, k), ch);
}

// the greatest row among those that carry that maximum (complete: a kernel boundary lies in between).
// The plane bit is tested again: the cleared word equals a rejected row's change of 0
__global__ __launch_bounds__(SEL_BLK) void flat_pick_kernel(const FanLatestParams L) {
  const FanParams &F = L.fan;
  const uint64_t w = (uint64_t)blockIdx.x * SEL_WAVES + uniform32(threadIdx.x >> 6);
  const uint64_t i = w * 64 + lane_id();
  if (i >= F.src.n) return;
  const uint64_t s = L.group[i];
  if (s == LAT_NONE) return;
  const uint64_t ch = F.src.cols.change[i];
  for (uint32_t k = 0; k < L.nf; k++)
    if (((flat_plane(F, L.f0 + k, w) >> lane_id()) & 1ull) && ch == *flat_state(L, s, k))
      lat_max(flat_state(L, s, k) + 1, i + 1);
}

// fan_count's geometry and outputs with the predicate "in the plane, and the row its group picked
// under this filter": the pass's planes and their workgroup counts are overwritten (each ballot word
// is read and rewritten by the one wave that owns its 64 rows)
__global__ __launch_bounds__(FAN_BLK) void flat_keep_kernel(const FanLatestParams L) {
  __shared__ uint32_t wcnt[DRP_FANOUT_MAX][FAN_WAVES];
  const FanParams &F = L.fan;
  const uint32_t wv = uniform32(threadIdx.x >> 6), lane = lane_id();
  const uint64_t word0 = (uint64_t)blockIdx.x * FAN_CHUNKS + wv * FAN_RPL;  // (< nwords: the grid is nwg)
  uint64_t s[FAN_RPL];
#pragma unroll
  for (uint32_t r = 0; r < FAN_RPL; r++) {
    const uint64_t i = (word0 + r) * 64 + lane;
    s[r] = i < F.src.n ? L.group[i] : LAT_NONE;
  }
  for (uint32_t k = 0; k < L.nf; k++) {  // (wave-uniform: nf is a launch argument)
    uint64_t *mrow = F.mask + (uint64_t)(L.f0 + k) * F.nwords + word0;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < FAN_RPL; r++) {
      const uint64_t i = (word0 + r) * 64 + lane;
      const bool keep = ((mrow[r] >> lane) & 1ull) && s[r] != LAT_NONE && flat_state(L, s[r], k)[1] == i + 1;
      const uint64_t b = __ballot(keep);
      if (lane == 0) mrow[r] = b;
      cnt += (uint32_t)__popcll(b);
    }
    if (lane == 0) wcnt[k][wv] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < L.nf) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t j = 0; j < FAN_WAVES; j++) t += wcnt[threadIdx.x][j];
    F.block_cnt[(uint64_t)(L.f0 + threadIdx.x) * F.nwg + blockIdx.x] = t;
  }
}

}  // namespace drp

using namespace drp;

// the power of two >= 2 n: the table is at most half full
static uint64_t lat_nslots(uint64_t n) {
  uint64_t c = 2;
  while (c < 2 * n) c <<= 1;
  return c;
}
// the table for n rows at `at` (to be zeroed)
static LatTable lat_table(void *at, uint64_t n, uint64_t hash_mask) {
  LatTable T;
  T.tab = static_cast<uint64_t *>(at);
  T.nslots = lat_nslots(n);
  T.hash_mask = hash_mask;
  // rows below 2^32 - 1 leave rep's high half to 32 bits of the hash (most foreign slots are passed
  // without a look at their row); beyond, rep is the row alone and every visit compares the rows
  T.tag_mask = n < 0xFFFFFFFFull ? 0xFFFFFFFF00000000ull : 0;
  return T;
}

extern "C" uint64_t drp_latest_scratch_bytes(uint64_t n) {
  return al(drp_select_scratch_bytes(n)) + al(n * 8) + lat_nslots(n) * 24;
}

extern "C" hipError_t drp_launch_latest(const SelectParams *Pp, const SelectBytes *fb, uint64_t hash_mask,
                                        void *scratch, hipStream_t st) {
  LatestParams L;
  L.sel = *Pp;
  const uint64_t n = L.sel.src.n;
  if (n == 0) return hipMemsetAsync(L.sel.n_selected, 0, 8, st);
  if (const hipError_t e = drp_select_place(&L.sel, fb, scratch, st)) return e;
  uint8_t *sc = static_cast<uint8_t *>(scratch) + al(drp_select_scratch_bytes(n));
  L.slot = reinterpret_cast<uint64_t *>(sc);
  L.t = lat_table(sc + al(n * 8), n, hash_mask);
  if (const hipError_t e = hipMemsetAsync(L.t.tab, 0, L.t.nslots * 24, st)) return e;
  const dim3 grid((uint32_t)((n + SEL_BLK - 1) / SEL_BLK)), blk(SEL_BLK);
  hipLaunchKernelGGL(lat_insert_kernel, grid, blk, 0, st, L);
  hipLaunchKernelGGL(lat_pick_kernel, grid, blk, 0, st, L);
  hipLaunchKernelGGL(lat_keep_kernel, grid, blk, 0, st, L);
  const hipError_t e = drp_launch_select_compact(&L.sel, st);
  drp_dbg_mark("latest", st);
  return e;
}

static uint32_t flat_pass(uint32_t nfilters, uint32_t pass) { return pass == 0 || pass > nfilters ? nfilters : pass; }

extern "C" uint64_t drp_fanout_latest_scratch_bytes(uint64_t n, uint32_t nfilters, uint32_t pass) {
  const uint64_t words = al((n + 63) / 64 * 8);
  return al(drp_fanout_scratch_bytes(n, nfilters)) + al(n * 8) + lat_nslots(n) * 8 + 2 * words +
         n * 16 * (uint64_t)flat_pass(nfilters, pass);
}

extern "C" hipError_t drp_launch_fanout_latest(const FanParams *Pp, uint64_t hash_mask, uint32_t pass, void *scratch,
                                               hipStream_t st) {
  FanLatestParams L;
  L.fan = *Pp;
  const uint64_t n = L.fan.src.n;
  if (n == 0) return hipSuccess;
  const uint32_t K = L.fan.nfilters;
  pass = flat_pass(K, pass);
  const uint64_t m = (n + 63) / 64, words = al(m * 8);
  uint8_t *sc = static_cast<uint8_t *>(scratch) + al(drp_fanout_scratch_bytes(n, K));
  L.group = reinterpret_cast<uint64_t *>(sc);
  L.t = lat_table(sc + al(n * 8), n, hash_mask);
  L.lead = L.t.tab + L.t.nslots;
  L.lead_base = L.lead + words / 8;
  L.state = L.lead_base + words / 8;
  if (const hipError_t e = hipMemsetAsync(L.t.tab, 0, L.t.nslots * 8, st)) return e;
  const dim3 grid((uint32_t)((n + SEL_BLK - 1) / SEL_BLK)), blk(SEL_BLK);
  L.f0 = L.nf = 0;
  hipLaunchKernelGGL(flat_group_kernel, grid, blk, 0, st, L);
  hipLaunchKernelGGL(flat_scan_kernel, dim3(1), blk, 0, st, L, m);
  hipLaunchKernelGGL(flat_number_kernel, grid, blk, 0, st, L);
  for (L.f0 = 0; L.f0 < K; L.f0 += pass) {
    L.nf = K - L.f0 < pass ? K - L.f0 : pass;
    // (the groups are at most n; how many there are stays on the device)
    if (const hipError_t e = hipMemsetAsync(L.state, 0, n * L.nf * 16, st)) return e;
    hipLaunchKernelGGL(flat_max_kernel, grid, blk, 0, st, L);
    hipLaunchKernelGGL(flat_pick_kernel, grid, blk, 0, st, L);
    hipLaunchKernelGGL(flat_keep_kernel, dim3((uint32_t)L.fan.nwg), dim3(FAN_BLK), 0, st, L);
  }
  drp_dbg_mark("fanout_latest", st);
  return hipGetLastError();
}
