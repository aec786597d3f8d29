// drp_keyorder.hip — gfx950 key-ordered listing: the encoder rows of every segment of a fan-out's
// output (drp_change_src over a heap, segment f = rows [row_base[f], row_base[f + 1])) put in ascending
// (key bytes, subset presence, subset bytes, input position), cut to a key range and a limit per
// segment, and laid end to end again. No reference counterpart (the reference has no relay); the fields
// read are `key` and `subset` of messages/schema.proto:1-8.
//
// A byte string orders as the tuple (its 8-byte words read big-endian and padded with zeros, its
// length): the words decide wherever two strings differ inside their common length, and where one is a
// prefix of the other the padding makes the words equal or the shorter one smaller, and the length
// separates "ab" from "ab\0". So the order is drp_order.hip's stable LSD radix sort of (64-bit word,
// row) pairs run once per field, least significant field first: subset length, subset words last to
// first, subset presence, key length, key words last to first, and last the segment.
//  (0) ord_init (drp_order.hip), then ordk_pre / ordk_prefin: per row the ranges checked (key, and
//      with DRP_F_SUBSET subset, inside the heap and at most DRP_KEYORDER_MAX_BYTES), the rows that
//      fail marked in `bad` and never read again; the identity permutation into pair buffer 1; the
//      longest key and subset and the counts, reduced per workgroup and then by one workgroup.
//      The host waits for the stream here, once: the longest key and subset say how many fields the
//      chain has, and a field nobody has (no subset anywhere, only empty keys) is not launched.
//      The same pass counts the leading whole key words that every row shares with the first row
//      (a common prefix, as under a key_prefix filter); those fields are not launched either: they
//      cost the reading of the prefix once, here. (DRP_ORDER_SKIP=0 launches them.)
//  (1) per field ordk_fetch: position e of the current order holds row idx[e]; its field value goes to
//      key[e] of the same pair buffer. For a word that is one load of 8 bytes at any alignment, byte
//      swapped and masked to the string's end; only where those 8 bytes would pass the heap's end the
//      (at most 7) bytes are read one by one. The lanes of a workgroup issue their four loads together.
//      The same kernel reduces the OR and the AND of the values it loaded, and ordk_plan, one
//      workgroup, switches off the digits in which no two values differ, as ord_plan does; a length
//      has two digits, a presence one, and the last word of the longest string only its upper digits.
//  (2) per active digit the four kernels of drp_order.hip's pass, unchanged. In the segment pass a row
//      marked bad sorts behind the others of its segment (digit 2 * segment + bad).
//  (3) ordk_cut: one lane per segment. The rows that took part end at the first bad one; lo and hi are
//      lower / upper bounds over the sorted segment by binary search (at most 33 steps of a word-wise
//      compare of at most 512 words); the limit; with DRP_KEYORDER_KEEP_TIES the end of the run of the
//      last kept key, by the same search against that row's key. out_base is the scan of the kept counts,
//      and seg_start[f] the position of segment f's first kept row.
//  (4) ord_gather (drp_order.hip).
// No global atomics; no lane waits for another; every loop is bounded; no byte at or beyond heap +
// heap_bytes is read; the result is a function of the input alone.
#include "drp_order.h"

namespace drp {

// Word w (bytes [8w, 8w + 8), big-endian, zeros past the end) of the string [off, off + len) of a
// heap of hb bytes; off + len <= hb. Reads inside [off, hb) only.
__device__ __forceinline__ uint64_t ordk_word(const uint8_t *heap, uint64_t hb, uint64_t off, uint32_t len, uint32_t w) {
  const uint32_t at = 8 * w;
  if (at >= len) return 0;
  const uint32_t nb = len - at < 8 ? len - at : 8;
  const uint64_t a = off + at;
  uint64_t v = 0;
  if (a + 8 <= hb) {
    __builtin_memcpy(&v, heap + a, 8);
    v = __builtin_bswap64(v);
  } else {
    for (uint32_t k = 0; k < 7 && k < nb; k++) v |= (uint64_t)heap[a + k] << (56 - 8 * k);  // (nb <= hb - a < 8)
  }
  return nb < 8 ? v & (~0ull << (8 * (8 - nb))) : v;
}

// the value of a field of a row that takes part
__device__ __forceinline__ uint64_t ordk_value(const KeyOrderParams &K, uint32_t kind, uint32_t w, uint64_t row) {
  const drp_change_src &R = K.o.rows;
  if (kind == ORDK_KEY_WORD) return ordk_word(K.heap, K.heap_bytes, R.key_off[row], R.key_len[row], w);
  if (kind == ORDK_KEY_LEN) return R.key_len[row];
  const bool has = R.flags[row] & DRP_F_SUBSET;
  if (kind == ORDK_SUB_HAS) return has;
  if (!has) return 0;
  if (kind == ORDK_SUB_LEN) return R.subset_len[row];
  return ordk_word(K.heap, K.heap_bytes, R.subset_off[row], R.subset_len[row], w);
}

__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
#pragma unroll
  for (uint32_t m = 1; m < WAVE; m <<= 1) {
    const uint32_t o = shfl_xor32(v, m);
    v = o > v ? o : v;
  }
  return v;
}

// what ordk_pre reduces: the longest key and subset, the rows left out, whether a subset is present,
// and the leading whole key words every row that takes part shares (at most ORDK_WORDS)
constexpr uint32_t ORDK_WORDS = DRP_KEYORDER_MAX_BYTES / 8;
struct OrdkSum {
  uint32_t mk, ms, nb, as, lc;
};
// over a workgroup of ORD_BLK threads, in thread 0 (sw: 5 * ORD_WAVES words of LDS)
__device__ __forceinline__ void ordk_block_sum(OrdkSum &s, uint32_t *sw) {
  s.mk = wave_max32(s.mk);
  s.ms = wave_max32(s.ms);
  s.nb = wave_sum32(s.nb);
  s.as = wave_max32(s.as);
  s.lc = ORDK_WORDS - wave_max32(ORDK_WORDS - s.lc);  // (the least)
  const uint32_t wv = threadIdx.x >> 6;
  if (lane_id() == 0) {
    sw[5 * wv] = s.mk;
    sw[5 * wv + 1] = s.ms;
    sw[5 * wv + 2] = s.nb;
    sw[5 * wv + 3] = s.as;
    sw[5 * wv + 4] = s.lc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t k = 1; k < ORD_WAVES; k++) {
      s.mk = sw[5 * k] > s.mk ? sw[5 * k] : s.mk;
      s.ms = sw[5 * k + 1] > s.ms ? sw[5 * k + 1] : s.ms;
      s.nb += sw[5 * k + 2];
      s.as |= sw[5 * k + 3];
      s.lc = sw[5 * k + 4] < s.lc ? sw[5 * k + 4] : s.lc;
    }
  }
}

// the row takes no part: a range outside the heap, or a string above the cap
__device__ __forceinline__ bool ordk_row_bad(const drp_change_src &R, uint64_t row, uint64_t hb) {
  const uint64_t ko = R.key_off[row], so = R.subset_off[row];
  const uint32_t kl = R.key_len[row], sl = R.subset_len[row];
  bool bad = kl > DRP_KEYORDER_MAX_BYTES || ko > hb || kl > hb - ko;
  if (R.flags[row] & DRP_F_SUBSET) bad = bad || sl > DRP_KEYORDER_MAX_BYTES || so > hb || sl > hb - so;
  return bad;
}

// (0a) the rows that take part, the identity permutation, a workgroup's lengths and counts
// (part_or: longest key << 32 | longest subset; part_and: shared words << 32 | rows left out << 1 | a
// subset present). The shared words are counted against the first row's key: word w is shared if it
// lies whole inside every key and equals the first row's (none if the first row takes no part).
__global__ __launch_bounds__(ORD_BLK) void ordk_pre_kernel(const KeyOrderParams K) {
  __shared__ uint32_t sw[5 * ORD_WAVES];
  const OrderParams &P = K.o;
  const uint64_t n = P.ctl->n, e0 = (uint64_t)blockIdx.x * ORD_TILE;
  if (e0 >= n) return;
  const uint64_t b0 = P.ctl->b0, hb = K.heap_bytes;
  const drp_change_src &R = P.rows;
  const bool ref_ok = !ordk_row_bad(R, b0, hb);
  const uint64_t ref_off = ref_ok ? R.key_off[b0] : 0;
  const uint32_t ref_len = ref_ok ? R.key_len[b0] : 0;
  OrdkSum s = {0, 0, 0, 0, ORDK_WORDS};
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    const uint64_t e = e0 + r * ORD_BLK + threadIdx.x;
    if (e >= n) continue;
    const uint64_t row = b0 + e;
    const bool bad = ordk_row_bad(R, row, hb);
    K.bad[row] = bad;
    P.idx[0][e] = (uint32_t)row;
    if (bad) {
      s.nb++;
      continue;
    }
    const uint64_t ko = R.key_off[row];
    const uint32_t kl = R.key_len[row];
    s.mk = kl > s.mk ? kl : s.mk;
    if (R.flags[row] & DRP_F_SUBSET) {
      const uint32_t sl = R.subset_len[row];
      s.ms = sl > s.ms ? sl : s.ms;
      s.as = 1;
    }
    const uint32_t whole = (kl < ref_len ? kl : ref_len) / 8, lim = whole < s.lc ? whole : s.lc;
    uint32_t w = 0;
    for (; w < lim && w < ORDK_WORDS; w++)
      if (ordk_word(K.heap, hb, ko, kl, w) != ordk_word(K.heap, hb, ref_off, ref_len, w)) break;
    s.lc = w;
  }
  ordk_block_sum(s, sw);
  if (threadIdx.x == 0) {
    P.part_or[blockIdx.x] = ((uint64_t)s.mk << 32) | s.ms;
    P.part_and[blockIdx.x] = ((uint64_t)s.lc << 32) | ((uint64_t)s.nb << 1) | s.as;
  }
}

// (0b) one workgroup: the whole input's lengths and counts; the order so far is pair buffer 1's
__global__ __launch_bounds__(ORD_BLK) void ordk_prefin_kernel(const KeyOrderParams K) {
  __shared__ uint32_t sw[5 * ORD_WAVES];
  const OrderParams &P = K.o;
  OrdCtl &c = *P.ctl;
  const uint64_t n = c.n, nwg = c.nwg;
  OrdkSum s = {0, 0, 0, 0, ORDK_WORDS};
  uint64_t left = 0;  // (a workgroup's count fits 32 bits, their sum is kept in 64 per thread)
  for (uint64_t k = threadIdx.x; k < nwg; k += ORD_BLK) {
    const uint64_t a = P.part_or[k], b = P.part_and[k];
    s.mk = (uint32_t)(a >> 32) > s.mk ? (uint32_t)(a >> 32) : s.mk;
    s.ms = (uint32_t)a > s.ms ? (uint32_t)a : s.ms;
    left += (uint32_t)b >> 1;
    s.as |= (uint32_t)b & 1u;
    s.lc = (uint32_t)(b >> 32) < s.lc ? (uint32_t)(b >> 32) : s.lc;
  }
  s.nb = (uint32_t)left;  // (n <= rows_cap < 2^32)
  ordk_block_sum(s, sw);
  if (threadIdx.x != 0) return;
  OrdkCtl &k = *K.kctl;
  k.took = n - s.nb;
  k.left = s.nb;
  k.max_key = s.mk;
  k.max_sub = s.ms;
  k.any_sub = s.as;
  k.shared_words = s.lc;
  c.final_src = 1;
  for (uint32_t p = 0; p < ORD_PASSES; p++) c.act[p] = 0;
  if (K.totals) {
    K.totals[0] = n - s.nb;
    K.totals[1] = s.nb;
  }
}

// (1a) field (kind, w) of every row, in the order reached so far, and the OR and AND of a workgroup's
__global__ __launch_bounds__(ORD_BLK) void ordk_fetch_kernel(const KeyOrderParams K, uint32_t kind, uint32_t w) {
  __shared__ uint64_t wo[ORD_WAVES], wa[ORD_WAVES];
  const OrderParams &P = K.o;
  const OrdCtl &c = *P.ctl;
  const uint64_t n = c.n, e0 = (uint64_t)blockIdx.x * ORD_TILE;
  if (e0 >= n) return;
  const uint32_t buf = c.final_src - 1;  // (1 or 2 since ordk_prefin)
  const uint32_t *idx = P.idx[buf];
  uint64_t *key = P.key[buf];
  uint32_t row[ORD_RPL];
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    const uint64_t e = e0 + r * ORD_BLK + threadIdx.x;
    row[r] = e < n ? idx[e] : 0;
  }
  uint64_t o = 0, a = ~0ull;
#pragma unroll
  for (uint32_t r = 0; r < ORD_RPL; r++) {
    const uint64_t e = e0 + r * ORD_BLK + threadIdx.x;
    if (e >= n) continue;
    const uint64_t v = P.bad[row[r]] ? 0 : ordk_value(K, kind, w, row[r]);
    key[e] = v;
    o |= v;
    a &= v;
  }
  ord_block_or_and(o, a, wo, wa);
  if (threadIdx.x == 0) {
    P.part_or[blockIdx.x] = o;
    P.part_and[blockIdx.x] = a;
  }
}

// (1b) one workgroup: of the digits [p_lo, p_hi) of the field just fetched, those that run, and the
// buffer each reads (ord_plan's rule, continued from where the order lies now). seg: no field was
// fetched; the segment pass runs.
__global__ __launch_bounds__(ORD_BLK) void ordk_plan_kernel(const KeyOrderParams K, uint32_t p_lo, uint32_t p_hi,
                                                            uint32_t seg) {
  __shared__ uint64_t wo[ORD_WAVES], wa[ORD_WAVES];
  const OrderParams &P = K.o;
  OrdCtl &c = *P.ctl;
  const uint64_t n = c.n, nwg = c.nwg;
  uint64_t o = 0, a = ~0ull;
  if (!seg)
    for (uint64_t k = threadIdx.x; k < nwg; k += ORD_BLK) {
      o |= P.part_or[k];
      a &= P.part_and[k];
    }
  ord_block_or_and(o, a, wo, wa);
  if (threadIdx.x != 0) return;
  const uint64_t diff = n ? o ^ a : 0;
  uint32_t cur = c.final_src;
  for (uint32_t p = 0; p < ORD_PASSES; p++) {
    uint32_t act;
    if (p < ORD_SEG_PASS) act = !seg && n != 0 && p >= p_lo && p < p_hi && (!P.skip || ((diff >> (8 * p)) & 0xFFu) != 0);
    else act = seg && n != 0;
    c.act[p] = act;
    c.src[p] = cur;
    if (act) cur = cur == 1 ? 2 : 1;
  }
  c.final_src = cur;
}

// the key of the row at sorted position s against the string [xo, xo + xl) of the heap (xh, xhb):
// < 0, 0, > 0
__device__ __forceinline__ int ordk_cmp(const KeyOrderParams &K, uint64_t row, const uint8_t *xh, uint64_t xhb,
                                        uint64_t xo, uint32_t xl) {
  const uint64_t ko = K.o.rows.key_off[row];
  const uint32_t kl = K.o.rows.key_len[row], m = kl < xl ? kl : xl, nw = (m + 7) / 8;
  for (uint32_t w = 0; w < nw && w < DRP_KEYORDER_MAX_BYTES / 8; w++) {
    const uint64_t a = ordk_word(K.heap, K.heap_bytes, ko, kl, w), b = ordk_word(xh, xhb, xo, xl, w);
    if (a != b) return a < b ? -1 : 1;
  }
  return kl < xl ? -1 : kl > xl ? 1 : 0;
}

// the first position in [a, b) whose key is greater than the string (strict), or not less (b: none);
// the rows at [a, b) take part and are sorted
__device__ __forceinline__ uint64_t ordk_first(const KeyOrderParams &K, uint32_t fs, uint64_t b0, uint64_t a, uint64_t b,
                                               bool strict, const uint8_t *xh, uint64_t xhb, uint64_t xo, uint32_t xl) {
  for (uint32_t k = 0; k < 33 && a < b; k++) {  // (b - a < 2^32)
    const uint64_t mid = a + ((b - a) >> 1);
    const int cmp = ordk_cmp(K, ord_row_at(K.o, fs, b0, mid), xh, xhb, xo, xl);
    if (strict ? cmp <= 0 : cmp < 0) a = mid + 1;
    else b = mid;
  }
  return a;
}

// (3) the rows every segment keeps, where they start, and where the outputs start
__global__ __launch_bounds__(64) void ordk_cut_kernel(const KeyOrderParams K, const OrdkPages G) {
  const OrderParams &P = K.o;
  const OrdCtl &c = *P.ctl;
  const uint32_t f = threadIdx.x, fs = c.final_src;
  const uint64_t b0 = c.b0;
  uint64_t kept = 0, start = 0;
  if (f < P.nseg && c.valid) {
    const uint64_t lo = P.row_base[f] - b0, cnt = P.row_base[f + 1] - P.row_base[f];
    uint64_t a = lo, b = lo + cnt;
    if (K.kctl->left) {  // the rows left out stand last: b is the first of them
      uint64_t x = a;
      for (uint32_t k = 0; k < 33 && x < b; k++) {
        const uint64_t mid = x + ((b - x) >> 1);
        if (P.bad[ord_row_at(P, fs, b0, mid)]) b = mid;
        else x = mid + 1;
      }
      b = x;
    }
    const uint32_t fl = G.flags[f];
    if (fl & (DRP_KEYPAGE_FROM | DRP_KEYPAGE_AFTER))
      a = ordk_first(K, fs, b0, a, b, fl & DRP_KEYPAGE_AFTER, K.bounds, K.bounds_bytes, G.lo_off[f], G.lo_len[f]);
    if (fl & DRP_KEYPAGE_UNTIL) b = ordk_first(K, fs, b0, a, b, false, K.bounds, K.bounds_bytes, G.hi_off[f], G.hi_len[f]);
    kept = umin64(b - a, G.limit[f]);  // (a <= b: both searches answer inside [a, b])
    if ((P.flags & DRP_KEYORDER_KEEP_TIES) && kept > 0 && kept < b - a) {
      const uint64_t v = ord_row_at(P, fs, b0, a + kept - 1);
      kept = ordk_first(K, fs, b0, a + kept, b, true, K.heap, K.heap_bytes, P.rows.key_off[v], P.rows.key_len[v]) - a;
    }
    start = a - lo;
  }
  if (f < P.nseg) K.kctl->start[f] = start;
  const uint64_t incl = wave_incl_scan64(kept);
  if (f < P.nseg) P.out_base[f + 1] = incl;
  if (f == 0) P.out_base[0] = 0;
}

}  // namespace drp

using namespace drp;

namespace {
struct OrdkLayout {
  OrdLayout ord;
  uint64_t bad, kctl, bounds, end;
  OrdkLayout(uint64_t cap, uint64_t bounds_bytes) : ord(cap) {
    bad = ord.end;
    kctl = bad + al(cap);
    bounds = kctl + al(sizeof(OrdkCtl));
    end = bounds + al(bounds_bytes);
  }
};
}  // namespace

extern "C" uint64_t drp_keyorder_scratch_bytes(uint64_t rows_cap, uint64_t bounds_bytes) {
  return OrdkLayout(rows_cap, bounds_bytes).end;
}

extern "C" hipError_t drp_launch_keyorder(const KeyOrderParams *Kp, const OrdkPages *pages, const uint8_t *bounds_host,
                                          uint64_t out_max, void *scratch, hipStream_t st) {
  KeyOrderParams K = *Kp;
  OrderParams &P = K.o;
  const OrdkLayout L(P.rows_cap, K.bounds_bytes);
  uint8_t *sc = static_cast<uint8_t *>(scratch);
  L.ord.place(P, scratch);
  K.bad = sc + L.bad;
  K.kctl = reinterpret_cast<OrdkCtl *>(sc + L.kctl);
  K.bounds = sc + L.bounds;
  P.bad = K.bad;
  P.seg_start = K.kctl->start;
  const dim3 tiles((uint32_t)L.ord.nwg), one(1), blk(ORD_BLK);
  if (K.bounds_bytes) {
    const hipError_t e = hipMemcpyAsync(sc + L.bounds, bounds_host, K.bounds_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
  }
  drp_launch_order_init(&P, st);
  hipLaunchKernelGGL(ordk_pre_kernel, tiles, blk, 0, st, K);
  hipLaunchKernelGGL(ordk_prefin_kernel, one, blk, 0, st, K);
  // the one host wait: the longest key and subset size the chain (and the bounds have left the host)
  struct {
    uint64_t took, left;
    uint32_t max_key, max_sub, any_sub, shared_words;
  } h;
  static_assert(sizeof h == 32 && offsetof(OrdkCtl, start) == 32, "the head of OrdkCtl");
  hipError_t e = hipMemcpyAsync(&h, K.kctl, sizeof h, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  auto field = [&](uint32_t kind, uint32_t w, uint32_t p_lo, uint32_t p_hi) {
    hipLaunchKernelGGL(ordk_fetch_kernel, tiles, blk, 0, st, K, kind, w);
    hipLaunchKernelGGL(ordk_plan_kernel, one, blk, 0, st, K, p_lo, p_hi, 0u);
    for (uint32_t p = p_lo; p < p_hi; p++) drp_launch_order_pass(&P, p, st);
  };
  // the words of strings of at most `longest` bytes, last to first; the last word's low digits are padding
  // and the first `shared` words are the same in every row that takes part: they order nothing
  auto words = [&](uint32_t kind, uint32_t longest, uint32_t shared) {
    const uint32_t nw = (longest + 7) / 8;
    for (uint32_t w = nw; w-- > shared;) field(kind, w, w == nw - 1 && longest % 8 ? 8 - longest % 8 : 0, 8);
  };
  if (h.took) {
    if (h.any_sub) {
      if (h.max_sub) {
        field(ORDK_SUB_LEN, 0, 0, 2);  // (a length is at most 4096 = 2^12)
        words(ORDK_SUB_WORD, h.max_sub, 0);
      }
      field(ORDK_SUB_HAS, 0, 0, 1);
    }
    if (h.max_key) {
      field(ORDK_KEY_LEN, 0, 0, 2);
      words(ORDK_KEY_WORD, h.max_key, P.skip ? h.shared_words : 0);
    }
  }
  if (h.took + h.left && (P.nseg > 1 || h.left)) {
    hipLaunchKernelGGL(ordk_plan_kernel, one, blk, 0, st, K, 0u, 0u, 1u);
    drp_launch_order_pass(&P, ORD_SEG_PASS, st);
  }
  drp_dbg_mark("keyorder_sort", st);
  hipLaunchKernelGGL(ordk_cut_kernel, one, dim3(64), 0, st, K, *pages);
  drp_launch_order_gather(&P, out_max, st);
  drp_dbg_mark("keyorder_gather", st);
  return hipGetLastError();
}
