// drp_store.hip — gfx950 kernels of the store (include/drp.h "store"): the latest Change per
// identity (subset presence, subset bytes, key bytes) over every batch merged so far, kept in
// caller-owned device memory as the rows of a decoded batch over an arena of payloads, plus an
// open-addressing table from identity to row. No reference counterpart: the reference has no relay;
// the fields read are those of messages/schema.proto:1-8.
//
// A merge starts from the winners drp_launch_latest (drp_latest.hip) leaves: one row per identity,
// so identities are distinct within a merge. That is what keeps the persistent table simple: it is
// only looked up against bytes that earlier kernels wrote, and new identities claim free slots with
// a bare compare-and-swap. The rule of drp_latest.hip holds: what one workgroup writes and another
// reads within one kernel goes through an agent-scope atomic (only the table words of st_claim);
// everything else crosses a kernel boundary.
//   st_lookup   one winner per lane: the identity's hash (lat_group's: XXH64 of the key, the subset's
//               merged in, the ctx's hash mask), a linear probe of the table with atomic loads (no
//               kernel of a merge writes the table before st_claim), on a tag match the lengths and
//               then the winner's wire bytes against the row's arena bytes (plain reads: written by
//               earlier launches). The outcome (inserted / replaced / unchanged / stale / skipped),
//               the store row or the first free slot of the probe, the bytes needed; within the
//               workgroup the winner's rank among the inserted and the bytes needed before it; per
//               workgroup the sums.
//   scan        drp_select.hip's scan over the workgroups' inserted counts and over their bytes.
//   st_verdict  one workgroup: the remaining sums, the totals against the capacities, the verdict
//               and the last-merge group of the info record. Every later kernel reads the verdict
//               and does nothing after a refusal.
//   st_claim    the inserted winners: row = rows + rank, then from the saved slot on a
//               compare-and-swap of 0 -> tag | row + 1 per slot until one takes place. A slot taken
//               meanwhile belongs to another identity (they are distinct), so nothing is compared;
//               no lane waits for another; the loop ends after nslots steps at the latest.
//   st_write    the inserted and replaced winners, ST_GRP = 16 lanes each: key | subset | value into
//               the arena at arena_used + the scanned prefix, 16 bytes per lane and step (256 bytes
//               per step: a 4 KB value takes 16, a 40-byte payload one, and four winners share a
//               wave), the allocation's tail zeroed; the group's first lane writes the columns.
//   st_commit   rows, arena_used, arena_dead, merges.
// With a report (include/drp.h "merge report") the rep_* steps follow: see "report" below.
// The lookup (include/drp.h "lookup") probes the table as st_lookup does (st_probe, one copy) and
// writes nothing into the store: see "lookup" below.
// The compact is the same shape: the live allocations' sizes and their prefix, the scan, the verdict
// with the commit (nothing later reads the old totals), the copy.
// The load and the rehash (include/drp.h "store lifecycle") are the merge's steps around two plans of
// their own, stl_plan and strh_enter, and one check, st_selfcheck: see "lifecycle" below.
#include "drp_select.h"  // (wire_has, bytes_eq; drp_device.h: xxh, ld_agent, the wave scans)

namespace drp {

enum : uint32_t { ST_NONE = 0, ST_INSERT = 1, ST_REPLACE = 2, ST_UNCHANGED = 3, ST_STALE = 4, ST_SKIPPED = 5 };

__device__ __forceinline__ uint32_t st_r16(uint32_t len) { return (len + 15u) & ~15u; }  // (len <= 2^32 - 16)

// store row r's payload lies inside the arena, at `at`, and holds an identity of `ident` bytes (key |
// subset)
__device__ __forceinline__ bool st_payload_ok(const StoreDev &S, uint64_t r, uint64_t ident, uint64_t &at) {
  at = S.payload_off[r];
  const uint64_t len = S.payload_len[r];
  if (len > S.arena_bytes || at > S.arena_bytes - len || ident > len) return false;
  return true;
}

// store row r (named by a table word) has this identity; a row outside the store, or whose payload
// leaves the arena (a table that no drp_store_init cleared), matches nothing and is never read
__device__ __forceinline__ bool st_same(const StoreDev &S, uint64_t r, bool has, const uint8_t *key, uint32_t klen,
                                        const uint8_t *sub, uint32_t slen) {
  if (r >= S.max_keys) return false;
  const drp_changes &c = S.cols;
  if (((c.flags[r] & DRP_F_SUBSET) != 0) != has || c.key_len[r] != klen || c.subset_len[r] != slen) return false;
  uint64_t at;
  if (!st_payload_ok(S, r, (uint64_t)klen + slen, at)) return false;
  const uint8_t *a = S.arena + at;
  return bytes_eq(a, key, klen) && bytes_eq(a + klen, sub, slen);
}

// the identity's hash: lat_group's (XXH64 of the key, the subset's merged in: an empty subset still
// changes it), under the ctx's hash mask
__device__ __forceinline__ uint64_t st_hash(const StoreDev &S, bool has, const uint8_t *key, uint32_t klen,
                                            const uint8_t *sub, uint32_t slen) {
  uint64_t h = xxh::xxh64(key, klen);
  if (has) h = xxh::merge(h, xxh::xxh64(sub, slen));
  return h & S.hash_mask;
}

// The probe of the table for an identity of hash h, one copy for the merge (st_lookup) and the
// read-only lookup (lk_probe): a linear walk with atomic loads to the next free slot or tag match,
// then (outside that loop) the byte compare of st_same. Nothing is written. Returns the store row
// that holds the identity, or ~0 with `free_slot` = the first free slot of the probe (~0 as well for
// a table without one: not reached, it is at most half full).
__device__ __forceinline__ uint64_t st_probe(const StoreDev &S, uint64_t h, bool has, const uint8_t *key,
                                             uint32_t klen, const uint8_t *sub, uint32_t slen, uint64_t &free_slot) {
  const uint64_t smask = S.nslots - 1;
  uint64_t s = h & smask, step = 0;
  free_slot = ~0ull;
  while (step < S.nslots) {
    uint64_t seen = 0;
    for (; step < S.nslots; step++, s = (s + 1) & smask) {
      seen = ld_agent(S.table + s);
      if (seen == 0 || ((seen ^ h) & ST_TAG) == 0) break;
    }
    if (step == S.nslots) break;
    if (seen == 0) {
      free_slot = s;
      break;
    }
    if (st_same(S, (seen & ~ST_TAG) - 1, has, key, klen, sub, slen)) return (seen & ~ST_TAG) - 1;
    step++;
    s = (s + 1) & smask;
  }
  return ~0ull;
}

// winner i of M as the plans read it (an absent field has length 0), and whether it can be stored:
// its three ranges inside the wire, its payload within an allocation's 2^32 - 16 bytes. One that
// cannot is never read (a latest's winner was a candidate, so its key and subset are inside; a
// select's row, and any winner's value, need not be)
struct StWinner {
  uint64_t koff, soff, voff, plen;
  uint32_t fl, klen, slen, vlen;
  bool has, ok;
};
__device__ __forceinline__ StWinner st_winner(const StoreMerge &M, uint64_t i) {
  StWinner w;
  w.fl = M.w.flags[i];
  w.has = (w.fl & DRP_F_SUBSET) != 0;
  const bool hv = (w.fl & DRP_F_VALUE) != 0;
  w.koff = M.w.key_off[i], w.soff = M.w.subset_off[i], w.voff = M.w.value_off[i];
  w.klen = M.w.key_len[i], w.slen = w.has ? M.w.subset_len[i] : 0, w.vlen = hv ? M.w.value_len[i] : 0;
  w.plen = (uint64_t)w.klen + w.slen + w.vlen;
  RowSrc W = {};
  W.nbytes = M.nbytes;
  w.ok = wire_has(W, w.koff, w.klen) && (!w.has || wire_has(W, w.soff, w.slen)) &&
         (!hv || wire_has(W, w.voff, w.vlen)) && w.plen <= 0xFFFFFFF0ull;
  return w;
}

// The plans' epilogue (st_lookup, stl_plan; every lane of the workgroup): winner i's state, within the
// workgroup its rank among the inserted and the bytes needed before it, per workgroup the sums
__device__ __forceinline__ void st_publish(const StoreMerge &M, uint64_t i, uint32_t code, uint32_t alloc,
                                           uint64_t where, uint64_t h, uint64_t dead) {
  __shared__ uint32_t wcnt[ST_WAVES][ST_MISC];
  __shared__ uint64_t wdead[ST_WAVES], sw[ST_WAVES];
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t bi = __ballot(code == ST_INSERT), br = __ballot(code == ST_REPLACE),
                 bu = __ballot(code == ST_UNCHANGED), bs = __ballot(code == ST_STALE),
                 bk = __ballot(code == ST_SKIPPED);
  const uint64_t dsum = wave_sum64(dead);
  if (lane == 0) {
    wcnt[wv][0] = (uint32_t)__popcll(bi);
    wcnt[wv][1] = (uint32_t)__popcll(br);
    wcnt[wv][2] = (uint32_t)__popcll(bu);
    wcnt[wv][3] = (uint32_t)__popcll(bs);
    wcnt[wv][4] = (uint32_t)__popcll(bk);
    wdead[wv] = dsum;
  }
  uint64_t btotal;
  const uint64_t before = block_excl_scan<uint64_t>(alloc, sw, btotal);  // (its barrier publishes wcnt and wdead too)
  uint32_t irank = (uint32_t)__popcll(bi & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wv; k++) irank += wcnt[k][0];
  M.where[i] = where;  // (i < nblk * ST_BLK: the state covers whole workgroups)
  M.hash[i] = h;
  M.boff[i] = before;
  M.alloc[i] = alloc;
  M.meta[i] = code | (irank << 8);
  if (threadIdx.x < ST_MISC + 1) {
    uint64_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < ST_WAVES; k++) t += threadIdx.x < ST_MISC ? (uint64_t)wcnt[k][threadIdx.x] : wdead[k];
    if (threadIdx.x == 0) {
      M.blk_ins[blockIdx.x] = t;
      M.blk_bytes[blockIdx.x] = btotal;
    } else {
      M.blk_misc[(uint64_t)blockIdx.x * ST_MISC + threadIdx.x - 1] = t;  // [4]: the dead bytes
    }
  }
}

__global__ __launch_bounds__(ST_BLK) void st_lookup_kernel(const StoreMerge M) {
  const StoreDev &S = M.s;
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  uint32_t code = ST_NONE, alloc = 0;
  uint64_t where = 0, h = 0, dead = 0;
  if (i < *M.nw && i < M.n) {
    const StWinner w = st_winner(M, i);
    const bool has = w.has;
    const uint32_t fl = w.fl, klen = w.klen, slen = w.slen, vlen = w.vlen;
    const uint64_t plen = w.plen;
    if (!w.ok) {
      code = ST_SKIPPED;
    } else {
      const uint8_t *key = M.bytes + w.koff, *sub = M.bytes + w.soff, *val = M.bytes + w.voff;
      h = st_hash(S, has, key, klen, sub, slen);
      uint64_t free_slot;
      const uint64_t r = st_probe(S, h, has, key, klen, sub, slen, free_slot);
      code = ST_SKIPPED;  // (a table without a free slot: not reached, it is at most half full)
      if (r == ~0ull && free_slot != ~0ull) {
        code = ST_INSERT;
        where = free_slot;
      }
      if (r != ~0ull) {
        const drp_changes &c = S.cols;
        const uint64_t sch = c.change[r], wch = M.w.change[i];
        where = r;
        if (sch > wch) {
          code = ST_STALE;
        } else if (sch == wch && c.from[r] == M.w.from[i] && c.to[r] == M.w.to[i] &&
                   (c.flags[r] & (DRP_F_SUBSET | DRP_F_VALUE)) == fl && c.value_len[r] == vlen &&
                   (uint64_t)S.payload_len[r] == plen &&
                   bytes_eq(S.arena + S.payload_off[r] + klen + slen, val, vlen)) {
          code = ST_UNCHANGED;
        } else {
          code = ST_REPLACE;
          dead = st_r16(S.payload_len[r]);
        }
      }
      if (code == ST_INSERT || code == ST_REPLACE) alloc = st_r16((uint32_t)plen);
    }
  }
  st_publish(M, i, code, alloc, where, h, dead);
}

// one workgroup: the sums the scans did not take, the verdict, the record's last-merge group
__global__ __launch_bounds__(ST_BLK) void st_verdict_kernel(const StoreMerge M) {
  __shared__ uint64_t part[ST_WAVES][ST_MISC];
  uint64_t s[ST_MISC] = {};
  for (uint64_t b = threadIdx.x; b < M.nblk; b += ST_BLK)
#pragma unroll
    for (uint32_t k = 0; k < ST_MISC; k++) s[k] += M.blk_misc[b * ST_MISC + k];
#pragma unroll
  for (uint32_t k = 0; k < ST_MISC; k++) {
    s[k] = wave_sum64(s[k]);
    if (lane_id() == 0) part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (uint32_t k = 0; k < ST_MISC; k++) {
    s[k] = 0;
    for (uint32_t w = 0; w < ST_WAVES; w++) s[k] += part[w][k];
  }
  drp_store_info *I = M.s.info;
  const uint64_t ins = M.ctl[0], bytes = M.ctl[1], nw = umin64(*M.nw, M.n);
  const uint64_t rows = umin64(I->rows, M.s.max_keys), used = umin64(I->arena_used, M.s.arena_bytes);
  I->winners = nw;
  I->inserted = ins;
  I->replaced = s[0];
  I->unchanged = s[1];
  I->stale = s[2];
  I->skipped = s[3];
  I->refused = (ins > M.s.max_keys - rows || bytes > M.s.arena_bytes - used) ? 1 : 0;
  I->need_rows = ins;
  I->need_bytes = bytes;
  M.ctl[2] = s[4];
}

// row `row` of hash h into the first free slot from s on (st_claim, strh_enter): a compare-and-swap
// of 0 -> tag | row + 1 per slot until one takes place, nslots steps at the latest
__device__ __forceinline__ void st_enter(const StoreDev &S, uint64_t s, uint64_t h, uint64_t row) {
  const uint64_t word = (h & ST_TAG) | (row + 1), smask = S.nslots - 1;
  s &= smask;
  for (uint64_t step = 0; step < S.nslots; step++, s = (s + 1) & smask) {
    uint64_t seen = 0;
    if (__hip_atomic_compare_exchange_strong(S.table + s, &seen, word, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      break;
  }
}

__global__ __launch_bounds__(ST_BLK) void st_claim_kernel(const StoreMerge M) {
  const StoreDev &S = M.s;
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  if (i >= *M.nw || i >= M.n || S.info->refused) return;
  const uint32_t meta = M.meta[i];
  if ((meta & 0xFF) != ST_INSERT) return;
  const uint64_t row = S.info->rows + M.blk_ins[blockIdx.x] + (meta >> 8);  // (< max_keys: the verdict)
  st_enter(S, M.where[i], M.hash[i], row);
  M.where[i] = row;  // (read by this winner's lanes of st_write only)
}

// bytes [p0, p0 + 16) of key | subset | value, zeros past its end
__device__ __forceinline__ uint4 st_chunk(const uint8_t *key, uint32_t klen, const uint8_t *sub, uint32_t slen,
                                          const uint8_t *val, uint32_t vlen, uint32_t p0) {
  const uint32_t ks = klen + slen, plen = ks + vlen;
  uint64_t lo = 0, hi = 0;
  if (p0 >= ks && p0 + 16 <= plen) {
    lo = xxh::rd64(val + (p0 - ks));
    hi = xxh::rd64(val + (p0 - ks) + 8);
  } else {
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) {
      const uint32_t p = p0 + b;
      uint64_t x = 0;
      if (p < klen) x = key[p];
      else if (p < ks) x = sub[p - klen];
      else if (p < plen) x = val[p - ks];
      if (b < 8) lo |= x << (8 * b);
      else hi |= x << (8 * (b - 8));
    }
  }
  return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

__global__ __launch_bounds__(ST_BLK) void st_write_kernel(const StoreMerge M) {
  const StoreDev &S = M.s;
  const uint64_t t = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x, i = t / ST_GRP;
  const uint32_t g = (uint32_t)(t % ST_GRP);
  if (i >= *M.nw || i >= M.n || S.info->refused) return;
  const uint32_t code = M.meta[i] & 0xFF;
  if (code != ST_INSERT && code != ST_REPLACE) return;
  const uint64_t row = M.where[i], at = S.info->arena_used + M.blk_bytes[i / ST_BLK] + M.boff[i];
  const uint32_t alloc = M.alloc[i];
  // (the verdict keeps both inside the store; a record a caller has overwritten must not lead outside)
  if (row >= S.max_keys || at > S.arena_bytes || alloc > S.arena_bytes - at) return;
  const uint32_t fl = M.w.flags[i];
  const uint32_t klen = M.w.key_len[i], slen = (fl & DRP_F_SUBSET) ? M.w.subset_len[i] : 0,
                 vlen = (fl & DRP_F_VALUE) ? M.w.value_len[i] : 0;
  const uint8_t *key = M.bytes + M.w.key_off[i], *sub = M.bytes + M.w.subset_off[i], *val = M.bytes + M.w.value_off[i];
  uint4 *dst = reinterpret_cast<uint4 *>(S.arena + at);  // (16-byte aligned: the arena is, and every allocation)
  for (uint32_t p0 = g * 16; p0 < alloc; p0 += ST_GRP * 16) dst[p0 >> 4] = st_chunk(key, klen, sub, slen, val, vlen, p0);
  if (g != 0) return;
  const drp_changes &c = S.cols;
  S.payload_off[row] = at;
  S.payload_len[row] = klen + slen + vlen;
  S.type[row] = DRP_TYPE_CHANGE;
  c.key_off[row] = 0;
  c.key_len[row] = klen;
  c.subset_off[row] = klen;
  c.subset_len[row] = slen;
  c.value_off[row] = klen + slen;
  c.value_len[row] = vlen;
  c.change[row] = M.w.change[i];
  c.from[row] = M.w.from[i];
  c.to[row] = M.w.to[i];
  c.flags[row] = (uint8_t)(fl & (DRP_F_SUBSET | DRP_F_VALUE));
}

__global__ void st_commit_kernel(const StoreMerge M) {
  drp_store_info *I = M.s.info;
  if (I->refused) return;
  I->rows += I->inserted;
  I->arena_used += I->need_bytes;
  I->arena_dead += M.ctl[2];
  I->merges += 1;
}

// ---- report -----------------------------------------------------------------------------------
// The steps behind st_commit that say which rows the counts of the record were (include/drp.h "merge
// report"). By then the verdict is in the record and where[i] of a stale winner is its store row.
//   rep_clear  the batch's n rows, REP_ROWS per lane: outcome zeroed, news_type zeroed or, with
//              DRP_REPORT_KEEP_BLOBS, the blob rows' type byte. A kernel of its own before rep_mark:
//              the winners' bytes lie anywhere among these, and two kernels order the two writes.
//   rep_mark   one winner per lane: outcome[row] = its code, news_type[row] = DRP_TYPE_CHANGE for an
//              inserted or replaced one unless the merge was refused. Winners have distinct rows.
//              The workgroup's stale count leaves blk_misc here (st_verdict has read it) for the scan.
//   scan       drp_select.hip's, over the workgroups' stale counts.
//   rep_reply  the stale winners: place = the scanned count + the rank among the workgroup's stale
//              winners (ballots and the waves' counts, as st_lookup ranks the inserted); if the total
//              fits reply_cap, the store row's ten columns as row_load / row_store write them.
constexpr uint32_t REP_ROWS = 16;

// the bytes of w whose low six bits are DRP_TYPE_BLOB, the others 0
__device__ __forceinline__ uint32_t rep_blobs(uint32_t w) {
  const uint32_t y = (w & 0x3F3F3F3Fu) ^ (0x01010101u * DRP_TYPE_BLOB);  // (a byte is 0 where it matches)
  const uint32_t nz = ((y + 0x7F7F7F7Fu) | y) & 0x80808080u;             // (y's bytes are < 0x40: no carry leaves one)
  return w & (((nz ^ 0x80808080u) >> 7) * 0xFFu);
}

// dst[0, n) = 0 or the blob bytes of src[0, n): chunk t of REP_ROWS bytes from dst's first 16-byte
// boundary on with one 16-byte store (src is read where it lies: unaligned), the bytes before that
// boundary and behind the last whole chunk one at a time by lane `nchunk`. Nothing at or beyond n.
__device__ __forceinline__ void rep_fill(uint8_t *dst, const uint8_t *src, uint64_t n, uint64_t t) {
  const uint64_t head = umin64(n, (16 - ((uintptr_t)dst & 15)) & 15), nchunk = (n - head) / REP_ROWS;
  if (t < nchunk) {
    const uint64_t at = head + t * REP_ROWS;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (src) {
      __builtin_memcpy(&v, src + at, 16);
      v = make_uint4(rep_blobs(v.x), rep_blobs(v.y), rep_blobs(v.z), rep_blobs(v.w));
    }
    *reinterpret_cast<uint4 *>(dst + at) = v;
  } else if (t == nchunk) {
    const uint64_t tail = head + nchunk * REP_ROWS;  // (n - tail < REP_ROWS)
    for (uint64_t k = 0; k < head; k++) dst[k] = src && (src[k] & 0x3F) == DRP_TYPE_BLOB ? src[k] : 0;
    for (uint64_t k = tail; k < n; k++) dst[k] = src && (src[k] & 0x3F) == DRP_TYPE_BLOB ? src[k] : 0;
  }
}

__global__ __launch_bounds__(ST_BLK) void rep_clear_kernel(const StoreReport R, uint64_t n) {
  const uint64_t t = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  if (R.outcome) rep_fill(R.outcome, nullptr, n, t);
  if (R.news_type) rep_fill(R.news_type, (R.flags & DRP_REPORT_KEEP_BLOBS) ? R.type : nullptr, n, t);
}

__global__ __launch_bounds__(ST_BLK) void rep_mark_kernel(const StoreMerge M, const StoreReport R) {
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  if (threadIdx.x == 0 && R.blk_stale) R.blk_stale[blockIdx.x] = M.blk_misc[(uint64_t)blockIdx.x * ST_MISC + 2];
  if (i >= *M.nw || i >= M.n || !R.src_row) return;
  const uint64_t r = R.src_row[i];
  if (r >= M.n) return;  // (not reached: a winner is a row of the batch)
  const uint32_t code = M.meta[i] & 0xFF;
  if (R.outcome) R.outcome[r] = (uint8_t)code;
  if (R.news_type && (code == ST_INSERT || code == ST_REPLACE) && !M.s.info->refused) R.news_type[r] = DRP_TYPE_CHANGE;
}

__global__ __launch_bounds__(ST_BLK) void rep_reply_kernel(const StoreMerge M, const StoreReport R) {
  __shared__ uint32_t wcnt[ST_WAVES];
  const StoreDev &S = M.s;
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  const bool stale = i < *M.nw && i < M.n && (M.meta[i] & 0xFF) == ST_STALE;
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t bs = __ballot(stale);
  if (lane == 0) wcnt[wv] = (uint32_t)__popcll(bs);
  __syncthreads();
  const uint64_t total = M.ctl[3];
  if (i == 0) *R.n_reply = total;
  if (!stale || total > R.reply_cap) return;
  uint64_t j = R.blk_stale[blockIdx.x] + (uint32_t)__popcll(bs & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wv; k++) j += wcnt[k];
  const uint64_t r = M.where[i];
  if (j >= R.reply_cap || r >= S.max_keys) return;  // (not reached: j < total, and a stale winner was found in a row)
  RowSrc V = {};  // the store's view (offsets absolute into the arena: no piece shift)
  V.payload_off = S.payload_off;
  V.cols = S.cols;
  row_store(R.reply, j, row_load(V, r), r);
}

// ---- lookup -----------------------------------------------------------------------------------
// The read-only probe (include/drp.h "lookup"): the batch's candidates are queries, each looked up by
// identity and compared by `change`; no byte of the store is written. Everything read here (the
// table, the columns, the arena) was written by earlier launches, nothing is handed between
// workgroups inside a kernel, and every store is a plain vector store.
//   (copy)     frames.type -> lack_type, max_keys bytes, on the stream before lk_probe.
//   lk_probe   one query per lane: sel_pred and the candidate's wire-range test, st_hash and st_probe
//              (the merge's), the verdict from the two changes; verdict / hit_row; a zero byte into
//              lack_type[row] for a hit whose change is not below the stored one (the only writes
//              behind the copy are zeros: the order of the queries decides nothing); the query's
//              rank among the workgroup's emitted queries (ballots and the waves' counts, as
//              st_lookup ranks the inserted); per workgroup the emitted count and the five verdict
//              counts.
//   scan       drp_select.hip's, over the workgroups' emitted counts.
//   lk_totals  one workgroup: the verdict counts summed over the workgroups, and *n_out.
//   lk_emit    the emitted queries, if their total fits rows_cap: place = the scanned count + the
//              rank; the store row's ten columns as row_load / row_store write them, as rep_reply.
__global__ __launch_bounds__(ST_BLK) void lk_probe_kernel(const StoreLookup Q) {
  __shared__ uint32_t wcnt[ST_WAVES][LK_CODES + 1];
  const StoreDev &S = Q.s;
  const RowSrc &P = Q.sel.src;
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  uint32_t code = DRP_LOOKUP_NONE;
  uint64_t row = ~0ull;
  if (i < P.n && sel_pred(Q.sel, i)) {
    const drp_changes &c = P.cols;
    const bool has = (c.flags[i] & DRP_F_SUBSET) != 0;
    const uint64_t base = P.payload_off[i] + row_shift(P, i);
    const uint64_t koff = base + c.key_off[i], soff = base + c.subset_off[i];
    const uint32_t klen = c.key_len[i], slen = has ? c.subset_len[i] : 0;
    // (lat_group's test: a row whose key or subset range leaves the wire is no candidate, never read)
    if (wire_has(P, koff, klen) && (!has || wire_has(P, soff, slen))) {
      const uint8_t *key = P.bytes + koff, *sub = P.bytes + soff;
      uint64_t free_slot;
      row = st_probe(S, st_hash(S, has, key, klen, sub, slen), has, key, klen, sub, slen, free_slot);
      if (row == ~0ull) {
        code = DRP_LOOKUP_ABSENT;
      } else {  // (row < max_keys: st_same)
        const uint64_t sch = S.cols.change[row], qch = c.change[i];
        code = sch > qch ? DRP_LOOKUP_AHEAD : sch == qch ? DRP_LOOKUP_LEVEL : DRP_LOOKUP_BEHIND;
        if (Q.lack_type && qch >= sch) Q.lack_type[row] = 0;
      }
    }
  }
  const bool in = i < P.n;
  if (in && Q.verdict) Q.verdict[i] = (uint8_t)code;
  if (in && Q.hit_row) Q.hit_row[i] = row;
  // the workgroup's sums, and this query's place among its emitted queries
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t be = __ballot(((Q.emit_mask >> code) & 1u) != 0);  // (bit 0 is never set: NONE is not emitted)
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t k = 0; k < LK_CODES; k++) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(in && code == k));
    if (lane == k + 1) mine = cnt;
  }
  if (lane == 0) mine = (uint32_t)__popcll(be);
  if (lane <= LK_CODES) wcnt[wv][lane] = mine;
  __syncthreads();
  if (Q.meta) {
    uint32_t rank = (uint32_t)__popcll(be & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < wv; k++) rank += wcnt[k][0];
    Q.where[i] = row;  // (i < nblk * ST_BLK: the state covers whole workgroups)
    Q.meta[i] = code | (rank << 8);
  }
  if (threadIdx.x <= LK_CODES) {
    uint64_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < ST_WAVES; k++) t += wcnt[k][threadIdx.x];
    if (threadIdx.x == 0) Q.blk_emit[blockIdx.x] = t;
    else Q.blk_cnt[(uint64_t)blockIdx.x * LK_CODES + threadIdx.x - 1] = t;
  }
}

// one workgroup: the verdict counts over all workgroups, and the emitted total the scan left
__global__ __launch_bounds__(ST_BLK) void lk_totals_kernel(const StoreLookup Q) {
  __shared__ uint64_t part[ST_WAVES][LK_CODES];
  uint64_t s[LK_CODES] = {};
  for (uint64_t b = threadIdx.x; b < Q.nblk; b += ST_BLK)
#pragma unroll
    for (uint32_t k = 0; k < LK_CODES; k++) s[k] += Q.blk_cnt[b * LK_CODES + k];
#pragma unroll
  for (uint32_t k = 0; k < LK_CODES; k++) {
    s[k] = wave_sum64(s[k]);
    if (lane_id() == 0) part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < LK_CODES && Q.counts) {
    uint64_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < ST_WAVES; w++) t += part[w][threadIdx.x];
    Q.counts[threadIdx.x] = t;
  }
  if (threadIdx.x == 0 && Q.n_out) *Q.n_out = Q.ctl[0];
}

__global__ __launch_bounds__(ST_BLK) void lk_emit_kernel(const StoreLookup Q) {
  const StoreDev &S = Q.s;
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  if (i >= Q.sel.src.n || Q.ctl[0] > Q.rows_cap) return;
  const uint32_t meta = Q.meta[i];
  if (!((Q.emit_mask >> (meta & 0xFF)) & 1u)) return;
  const uint64_t j = Q.blk_emit[blockIdx.x] + (meta >> 8), r = Q.where[i];
  if (j >= Q.rows_cap || r >= S.max_keys) return;  // (not reached: j < the total, and an emitted query was found in a row)
  RowSrc V = {};  // the store's view (offsets absolute into the arena: no piece shift)
  V.payload_off = S.payload_off;
  V.cols = S.cols;
  row_store(Q.out, j, row_load(V, r), i);
}

// ---- compact ----------------------------------------------------------------------------------
struct StoreCompact {
  StoreDev s;
  uint8_t *arena2;
  uint64_t arena2_bytes;
  uint64_t *boff;       // per row: the live bytes of its workgroup's rows before it
  uint64_t *blk_bytes;  // per workgroup of ST_BLK rows: its live bytes (scanned in place)
  uint64_t *ctl;        // [0] the live total
};

__global__ __launch_bounds__(ST_BLK) void stc_size_kernel(const StoreCompact Q) {
  const uint64_t r = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  const uint64_t rows = umin64(Q.s.info->rows, Q.s.max_keys);
  __shared__ uint64_t sw[ST_WAVES];
  uint64_t total;
  const uint64_t before = block_excl_scan<uint64_t>(r < rows ? st_r16(Q.s.payload_len[r]) : 0, sw, total);
  if (r < rows) Q.boff[r] = before;
  if (threadIdx.x == 0) Q.blk_bytes[blockIdx.x] = total;
}

__global__ void stc_verdict_kernel(const StoreCompact Q) {
  drp_store_info *I = Q.s.info;
  const uint64_t live = Q.ctl[0];
  I->winners = I->inserted = I->replaced = I->unchanged = I->stale = I->skipped = 0;
  I->need_rows = 0;
  I->need_bytes = live;
  I->refused = live > Q.arena2_bytes ? 1 : 0;
  if (I->refused) return;
  I->arena_used = live;
  I->arena_dead = 0;
}

// ST_GRP lanes per row, 16 bytes per lane and step (both ends are 16-byte aligned); every lane reads
// the row's old offset before the group's first lane, in the same wave, stores the new one
__global__ __launch_bounds__(ST_BLK) void stc_copy_kernel(const StoreCompact Q) {
  const StoreDev &S = Q.s;
  const uint64_t t = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x, r = t / ST_GRP;
  const uint32_t g = (uint32_t)(t % ST_GRP);
  if (r >= umin64(S.info->rows, S.max_keys) || S.info->refused) return;
  const uint64_t from = S.payload_off[r], to = Q.blk_bytes[r / ST_BLK] + Q.boff[r];
  const uint64_t alloc = st_r16(S.payload_len[r]);
  if ((from & 15) || from > S.arena_bytes || alloc > S.arena_bytes - from) return;  // (not a row of ours)
  if (to > Q.arena2_bytes || alloc > Q.arena2_bytes - to) return;                   // (not reached: the verdict)
  const uint4 *src = reinterpret_cast<const uint4 *>(S.arena + from);
  uint4 *dst = reinterpret_cast<uint4 *>(Q.arena2 + to);
  for (uint64_t k = g; k < alloc / 16; k += ST_GRP) dst[k] = src[k];
  if (g == 0) S.payload_off[r] = to;
}

// ---- lifecycle --------------------------------------------------------------------------------
// The load and the rehash (include/drp.h "store lifecycle"). Both enter rows whose identities the
// caller promises to be distinct, so nothing is looked up: a row goes to the first free slot from its
// home slot on (st_enter, st_claim's loop). The table words are still all that crosses workgroups
// inside a kernel; the counts below are only added to, and read after the kernel's end.
//   stl_plan     st_lookup's place in a load, one selected row per lane: skipped if a range leaves the
//                wire, else inserted; the hash, the home slot, the allocation; st_publish as st_lookup.
//                The scans, st_verdict, st_claim, st_write and st_commit follow unchanged.
//   strh_enter   one store row per lane over the zeroed table: a row st_same would not read is counted
//                and left out, every other enters under its hash from its arena bytes.
//   st_selfcheck one store row per lane (a load's new rows behind st_commit, or all rows): st_probe for
//                the row's own identity, counted if it names another row. A kernel of its own behind
//                the one that entered the rows: by then the table is final, and of two rows of one
//                identity every probe meets the one in the earlier slot first, so exactly the other is
//                counted, whichever won the race for it.
//   strh_finish  the record's last-merge group.

// the lanes of the workgroup with `flag`, added to *dst (null: not counted): the waves' ballots, their
// counts in LDS, one agent-scope add per workgroup that has any. Once per kernel, by every lane
__device__ __forceinline__ void st_count(bool flag, uint64_t *dst) {
  __shared__ uint32_t wcnt[ST_WAVES];
  const uint64_t b = __ballot(flag);
  if (lane_id() == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x != 0 || !dst) return;
  uint64_t t = 0;
#pragma unroll
  for (uint32_t k = 0; k < ST_WAVES; k++) t += wcnt[k];
  if (t) __hip_atomic_fetch_add(dst, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// store row r's own identity out of its columns and arena bytes, and its hash; false (nothing of the
// arena is read): a row that fails st_same's validity test
struct StOwn {
  const uint8_t *key, *sub;
  uint32_t klen, slen;
  bool has;
  uint64_t h;
};
__device__ __forceinline__ bool st_own(const StoreDev &S, uint64_t r, StOwn &d) {
  const drp_changes &c = S.cols;
  d.klen = c.key_len[r];
  d.slen = c.subset_len[r];
  d.has = (c.flags[r] & DRP_F_SUBSET) != 0;
  uint64_t at;
  if (!st_payload_ok(S, r, (uint64_t)d.klen + d.slen, at)) return false;
  d.key = S.arena + at;
  d.sub = d.key + d.klen;
  d.h = st_hash(S, d.has, d.key, d.klen, d.sub, d.slen);
  return true;
}

__global__ __launch_bounds__(ST_BLK) void stl_plan_kernel(const StoreMerge M) {
  const uint64_t i = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  uint32_t code = ST_NONE, alloc = 0;
  uint64_t h = 0;
  if (i < *M.nw && i < M.n) {
    const StWinner w = st_winner(M, i);
    code = ST_SKIPPED;
    if (w.ok) {
      code = ST_INSERT;
      h = st_hash(M.s, w.has, M.bytes + w.koff, w.klen, M.bytes + w.soff, w.slen);
      alloc = st_r16((uint32_t)w.plen);
    }
  }
  st_publish(M, i, code, alloc, h & (M.s.nslots - 1), h, 0);
}

__global__ __launch_bounds__(ST_BLK) void strh_enter_kernel(const StoreDev S, uint64_t *invalid) {
  const uint64_t r = (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  bool bad = false;
  if (r < umin64(S.info->rows, S.max_keys)) {
    StOwn d;
    bad = !st_own(S, r, d);
    if (!bad) st_enter(S, d.h, d.h, r);
  }
  st_count(bad, invalid);
}

// rows [first, rows): first = 0, or with `loaded` the rows before the load st_commit has just applied
// (a refused load added none)
__global__ __launch_bounds__(ST_BLK) void st_selfcheck_kernel(const StoreDev S, uint64_t *count, uint32_t loaded) {
  const drp_store_info *I = S.info;
  const uint64_t rows = umin64(I->rows, S.max_keys);
  const uint64_t first = !loaded ? 0 : I->refused ? rows : rows - umin64(I->inserted, rows);
  const uint64_t r = first + (uint64_t)blockIdx.x * ST_BLK + threadIdx.x;
  bool other = false;
  StOwn d;
  if (r < rows && st_own(S, r, d)) {
    uint64_t free_slot;
    other = st_probe(S, d.h, d.has, d.key, d.klen, d.sub, d.slen, free_slot) != r;
  }
  st_count(other, count);
}

__global__ void strh_finish_kernel(const StoreDev S, const uint64_t *report) {
  drp_store_info *I = S.info;
  I->winners = I->inserted = I->replaced = I->unchanged = I->stale = I->skipped = 0;
  I->need_rows = I->need_bytes = 0;
  I->refused = (report && (report[0] | report[1])) ? 1 : 0;
}

}  // namespace drp

using namespace drp;

static uint64_t st_nblk(uint64_t n) { return n ? (n + ST_BLK - 1) / ST_BLK : 1; }

extern "C" uint64_t drp_store_nslots(uint64_t max_keys) {
  if (max_keys == 0 || max_keys > (1ull << 31)) return 0;
  uint64_t c = 2;
  while (c < 2 * max_keys) c <<= 1;
  return c;
}

extern "C" hipError_t drp_launch_store_init(const StoreDev *S, hipStream_t st) {
  if (const hipError_t e = hipMemsetAsync(S->table, 0, S->nslots * 8, st)) return e;
  if (const hipError_t e = hipMemsetAsync(S->info, 0, sizeof(drp_store_info), st)) return e;
  return hipMemsetAsync(S->type, 0, S->max_keys, st);
}

// the merge's state: three 8-byte and two 4-byte words per winner (32 bytes per row of the batch,
// for whole workgroups), 2 + ST_MISC words per workgroup, the control words
extern "C" uint64_t drp_store_merge_scratch_bytes(uint64_t n) {
  const uint64_t nblk = st_nblk(n), m = nblk * ST_BLK;
  return 3 * al(m * 8) + 2 * al(m * 4) + 2 * al(nblk * 8) + al(nblk * ST_MISC * 8) + 256;
}

extern "C" uint64_t drp_store_blocks(uint64_t n) { return st_nblk(n); }

// M's state into `scratch`; false: more workgroups than a grid of st_write holds
static bool st_place(StoreMerge &M, void *scratch) {
  const uint64_t nblk = st_nblk(M.n), m = nblk * ST_BLK;
  if (nblk >= (1ull << 31) / ST_GRP) return false;
  uint8_t *sc = static_cast<uint8_t *>(scratch);
  auto take = [&](uint64_t bytes) { void *p = sc; sc += al(bytes); return p; };
  M.where = static_cast<uint64_t *>(take(m * 8));
  M.hash = static_cast<uint64_t *>(take(m * 8));
  M.boff = static_cast<uint64_t *>(take(m * 8));
  M.alloc = static_cast<uint32_t *>(take(m * 4));
  M.meta = static_cast<uint32_t *>(take(m * 4));
  M.blk_ins = static_cast<uint64_t *>(take(nblk * 8));
  M.blk_bytes = static_cast<uint64_t *>(take(nblk * 8));
  M.blk_misc = static_cast<uint64_t *>(take(nblk * ST_MISC * 8));
  M.ctl = static_cast<uint64_t *>(take(256));
  M.nblk = nblk;
  return true;
}

// what follows a plan (st_lookup, stl_plan): the scans, the verdict, the claims, the writes, the commit
static hipError_t st_apply(const StoreMerge &M, hipStream_t st) {
  const dim3 grid((uint32_t)M.nblk), blk(ST_BLK);
  if (const hipError_t e = drp_launch_count_scan(M.blk_ins, M.nblk, M.ctl + 0, st)) return e;
  if (const hipError_t e = drp_launch_count_scan(M.blk_bytes, M.nblk, M.ctl + 1, st)) return e;
  hipLaunchKernelGGL(st_verdict_kernel, dim3(1), blk, 0, st, M);
  hipLaunchKernelGGL(st_claim_kernel, grid, blk, 0, st, M);
  hipLaunchKernelGGL(st_write_kernel, dim3((uint32_t)(M.nblk * ST_GRP)), blk, 0, st, M);
  hipLaunchKernelGGL(st_commit_kernel, dim3(1), dim3(1), 0, st, M);
  return hipSuccess;
}

extern "C" hipError_t drp_launch_store_load(const StoreMerge *Mp, uint64_t *clash, void *scratch, hipStream_t st) {
  StoreMerge M = *Mp;
  if (!st_place(M, scratch)) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)M.nblk), blk(ST_BLK);
  hipLaunchKernelGGL(stl_plan_kernel, grid, blk, 0, st, M);
  if (const hipError_t e = st_apply(M, st)) return e;
  if (clash) {
    if (const hipError_t e = hipMemsetAsync(clash, 0, 8, st)) return e;
    hipLaunchKernelGGL(st_selfcheck_kernel, grid, blk, 0, st, M.s, clash, 1u);
  }
  drp_dbg_mark("store_load", st);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_store_rehash(const StoreDev *S, uint64_t *report, hipStream_t st) {
  if (const hipError_t e = hipMemsetAsync(S->table, 0, S->nslots * 8, st)) return e;
  if (report)
    if (const hipError_t e = hipMemsetAsync(report, 0, 16, st)) return e;
  const dim3 grid((uint32_t)st_nblk(S->max_keys)), blk(ST_BLK);
  hipLaunchKernelGGL(strh_enter_kernel, grid, blk, 0, st, *S, report);
  if (report) hipLaunchKernelGGL(st_selfcheck_kernel, grid, blk, 0, st, *S, report + 1, 0u);
  hipLaunchKernelGGL(strh_finish_kernel, dim3(1), dim3(1), 0, st, *S, (const uint64_t *)report);
  drp_dbg_mark("store_rehash", st);
  return hipGetLastError();
}

extern "C" hipError_t drp_launch_store_merge(const StoreMerge *Mp, const StoreReport *R, void *scratch,
                                             hipStream_t st) {
  StoreMerge M = *Mp;
  if (!st_place(M, scratch)) return hipErrorInvalidValue;
  const uint64_t nblk = M.nblk;
  const dim3 grid((uint32_t)nblk), blk(ST_BLK);
  hipLaunchKernelGGL(st_lookup_kernel, grid, blk, 0, st, M);
  if (const hipError_t e = st_apply(M, st)) return e;
  drp_dbg_mark("store_merge", st);
  if (R) {
    const bool rows = R->src_row && (R->outcome || R->news_type), reply = R->n_reply && R->blk_stale;
    if (rows && M.n) {
      const uint64_t lanes = M.n / REP_ROWS + 1;  // (the chunks, and the lane behind them for the ends)
      hipLaunchKernelGGL(rep_clear_kernel, dim3((uint32_t)((lanes + ST_BLK - 1) / ST_BLK)), blk, 0, st, *R, M.n);
    }
    if (rows || reply) hipLaunchKernelGGL(rep_mark_kernel, grid, blk, 0, st, M, *R);
    if (reply) {
      if (const hipError_t e = drp_launch_count_scan(R->blk_stale, nblk, M.ctl + 3, st)) return e;
      hipLaunchKernelGGL(rep_reply_kernel, grid, blk, 0, st, M, *R);
    }
    drp_dbg_mark("store_report", st);
  }
  return hipGetLastError();
}

// the lookup's state: the filter's byte strings, per query (for whole workgroups) an 8-byte and a
// 4-byte word, per workgroup 1 + LK_CODES words, the control words
extern "C" uint64_t drp_store_lookup_scratch_bytes(uint64_t n) {
  const uint64_t nblk = st_nblk(n), m = nblk * ST_BLK;
  return 2 * DRP_SEL_MAX_BYTES + al(m * 8) + al(m * 4) + al(nblk * 8) + al(nblk * LK_CODES * 8) + 256;
}

extern "C" hipError_t drp_launch_store_lookup(const StoreLookup *Qp, const SelectBytes *fb, void *scratch,
                                              hipStream_t st) {
  StoreLookup Q = *Qp;
  const uint64_t n = Q.sel.src.n, nblk = st_nblk(n), m = nblk * ST_BLK;
  if (nblk >= (1ull << 31)) return hipErrorInvalidValue;
  // (only the filter's byte strings are placed: the lookup reads neither ballot words nor counts)
  if (const hipError_t e = drp_select_place(&Q.sel, fb, scratch, st)) return e;
  uint8_t *sc = static_cast<uint8_t *>(scratch) + 2 * DRP_SEL_MAX_BYTES;
  auto take = [&](uint64_t bytes) { void *p = sc; sc += al(bytes); return p; };
  const bool emit = Q.n_out != nullptr;  // (the entry point passes out arrays only with n_out)
  Q.where = static_cast<uint64_t *>(take(m * 8));
  Q.meta = static_cast<uint32_t *>(take(m * 4));
  if (!emit) Q.where = nullptr, Q.meta = nullptr;
  Q.blk_emit = static_cast<uint64_t *>(take(nblk * 8));
  Q.blk_cnt = static_cast<uint64_t *>(take(nblk * LK_CODES * 8));
  Q.ctl = static_cast<uint64_t *>(take(256));
  Q.nblk = nblk;
  if (Q.lack_type)
    if (const hipError_t e = hipMemcpyAsync(Q.lack_type, Q.s.type, Q.s.max_keys, hipMemcpyDeviceToDevice, st)) return e;
  const dim3 grid((uint32_t)nblk), blk(ST_BLK);
  hipLaunchKernelGGL(lk_probe_kernel, grid, blk, 0, st, Q);
  if (emit)
    if (const hipError_t e = drp_launch_count_scan(Q.blk_emit, nblk, Q.ctl, st)) return e;
  if (emit || Q.counts) hipLaunchKernelGGL(lk_totals_kernel, dim3(1), blk, 0, st, Q);
  if (emit && Q.rows_cap) hipLaunchKernelGGL(lk_emit_kernel, grid, blk, 0, st, Q);
  drp_dbg_mark("store_lookup", st);
  return hipGetLastError();
}

extern "C" uint64_t drp_store_compact_scratch_bytes(uint64_t max_keys) {
  return al(max_keys * 8) + al(st_nblk(max_keys) * 8) + 256;
}

extern "C" hipError_t drp_launch_store_compact(const StoreDev *S, uint8_t *arena2, uint64_t arena2_bytes,
                                               void *scratch, hipStream_t st) {
  StoreCompact Q;
  Q.s = *S;
  Q.arena2 = arena2;
  Q.arena2_bytes = arena2_bytes;
  const uint64_t nblk = st_nblk(S->max_keys);
  uint8_t *sc = static_cast<uint8_t *>(scratch);
  Q.boff = reinterpret_cast<uint64_t *>(sc);
  Q.blk_bytes = reinterpret_cast<uint64_t *>(sc + al(S->max_keys * 8));
  Q.ctl = Q.blk_bytes + al(nblk * 8) / 8;
  const dim3 blk(ST_BLK);
  hipLaunchKernelGGL(stc_size_kernel, dim3((uint32_t)nblk), blk, 0, st, Q);
  if (const hipError_t e = drp_launch_count_scan(Q.blk_bytes, nblk, Q.ctl, st)) return e;
  hipLaunchKernelGGL(stc_verdict_kernel, dim3(1), dim3(1), 0, st, Q);
  hipLaunchKernelGGL(stc_copy_kernel, dim3((uint32_t)(nblk * ST_GRP)), blk, 0, st, Q);
  drp_dbg_mark("store_compact", st);
  return hipGetLastError();
}
