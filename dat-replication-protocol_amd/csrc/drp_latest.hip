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
#include "drp_select.h"

namespace drp {

// the three words of slot s
__device__ __forceinline__ uint64_t *lat_word(const LatestParams &L, uint64_t s, uint32_t w) { return L.tab + 3 * s + w; }

// wire bytes [a, a + len) == [b, b + len) (both ranges inside the wire)
__device__ __forceinline__ bool lat_bytes_eq(const RowSrc &P, uint64_t a, uint64_t b, uint32_t len) {
  const uint8_t *x = P.bytes + a, *y = P.bytes + b;
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

__global__ __launch_bounds__(SEL_BLK) void lat_insert_kernel(const LatestParams L) {
  const RowSrc &P = L.sel.src;
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  if (i >= P.n) return;
  uint64_t mine = LAT_NONE;
  if (sel_pred(L.sel, i)) {
    const drp_changes &c = P.cols;
    const bool has = (c.flags[i] & DRP_F_SUBSET) != 0;
    const uint64_t base = P.payload_off[i] + row_shift(P, i);
    const uint64_t koff = base + c.key_off[i], soff = base + c.subset_off[i];
    const uint32_t klen = c.key_len[i], slen = has ? c.subset_len[i] : 0;
    // a row whose key or subset range leaves the wire is never read and is no candidate
    if (wire_has(P, koff, klen) && (!has || wire_has(P, soff, slen))) {
      uint64_t h = xxh::xxh64(P.bytes + koff, klen);
      if (has) h = xxh::merge(h, xxh::xxh64(P.bytes + soff, slen));  // (an empty subset still changes h)
      h &= L.hash_mask;
      const uint64_t smask = L.nslots - 1, word = (h & L.tag_mask) | (i + 1);
      uint64_t s = h & smask;
      for (uint64_t step = 0; step < L.nslots; step++, s = (s + 1) & smask) {
        // rep is written once, so an atomic load that finds it set saves the swap (a stale 0 only
        // costs the swap, which leaves the word it found in `seen`)
        uint64_t seen = ld_agent(lat_word(L, s, 0));
        if (seen == 0 && __hip_atomic_compare_exchange_strong(lat_word(L, s, 0), &seen, word, __ATOMIC_RELAXED,
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          mine = s;
          break;
        }
        if (((seen ^ word) & L.tag_mask) == 0 && lat_same(P, (seen & ~L.tag_mask) - 1, has, koff, klen, soff, slen)) {
          mine = s;
          break;
        }
      }
      // the maximum only grows: a load that already shows the row's change or more saves the atomic
      // (a stale, smaller value only costs it), which is what keeps a hot key's rows off one address
      const uint64_t ch = c.change[i];
      if (mine != LAT_NONE && ld_agent(lat_word(L, mine, 1)) < ch)
        __hip_atomic_fetch_max(lat_word(L, mine, 1), ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  L.slot[i] = mine;
}

__global__ __launch_bounds__(SEL_BLK) void lat_pick_kernel(const LatestParams L) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  if (i >= L.sel.src.n) return;
  const uint64_t s = L.slot[i];
  if (s == LAT_NONE) return;
  // (a group whose only change is 0 matches the cleared word)
  if (L.sel.src.cols.change[i] == *lat_word(L, s, 1) && ld_agent(lat_word(L, s, 2)) < i + 1)  // (as lat_insert's maximum)
    __hip_atomic_fetch_max(lat_word(L, s, 2), i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sel_count_kernel with the predicate "the row its group picked"
__global__ __launch_bounds__(SEL_BLK) void lat_keep_kernel(const LatestParams L) {
  const uint64_t i = (uint64_t)blockIdx.x * SEL_BLK + threadIdx.x;
  bool keep = false;
  if (i < L.sel.src.n) {
    const uint64_t s = L.slot[i];
    keep = s != LAT_NONE && *lat_word(L, s, 2) == i + 1;
  }
  sel_publish(L.sel, keep);
}

}  // namespace drp

using namespace drp;

static uint64_t lat_al(uint64_t x) { return (x + 255) & ~255ull; }
// the power of two >= 2 n: the table is at most half full
static uint64_t lat_nslots(uint64_t n) {
  uint64_t c = 2;
  while (c < 2 * n) c <<= 1;
  return c;
}
extern "C" uint64_t drp_latest_scratch_bytes(uint64_t n) {
  return lat_al(drp_select_scratch_bytes(n)) + lat_al(n * 8) + lat_nslots(n) * 24;
}

extern "C" hipError_t drp_launch_latest(const SelectParams *Pp, const SelectBytes *fb, uint64_t hash_mask,
                                        void *scratch, hipStream_t st) {
  LatestParams L;
  L.sel = *Pp;
  const uint64_t n = L.sel.src.n;
  if (n == 0) return hipMemsetAsync(L.sel.n_selected, 0, 8, st);
  if (const hipError_t e = drp_select_place(&L.sel, fb, scratch, st)) return e;
  uint8_t *sc = static_cast<uint8_t *>(scratch) + lat_al(drp_select_scratch_bytes(n));
  L.slot = reinterpret_cast<uint64_t *>(sc);
  L.tab = reinterpret_cast<uint64_t *>(sc + lat_al(n * 8));
  L.nslots = lat_nslots(n);
  L.hash_mask = hash_mask;
  // rows below 2^32 - 1 leave rep's high half to 32 bits of the hash (most foreign slots are passed
  // without a look at their row); beyond, rep is the row alone and every visit compares the rows
  L.tag_mask = n < 0xFFFFFFFFull ? 0xFFFFFFFF00000000ull : 0;
  if (const hipError_t e = hipMemsetAsync(L.tab, 0, L.nslots * 24, st)) return e;
  const dim3 grid((uint32_t)((n + SEL_BLK - 1) / SEL_BLK)), blk(SEL_BLK);
  hipLaunchKernelGGL(lat_insert_kernel, grid, blk, 0, st, L);
  hipLaunchKernelGGL(lat_pick_kernel, grid, blk, 0, st, L);
  hipLaunchKernelGGL(lat_keep_kernel, grid, blk, 0, st, L);
  const hipError_t e = drp_launch_select_compact(&L.sel, st);
  drp_dbg_mark("latest", st);
  return e;
}
