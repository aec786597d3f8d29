// drp_relay.hip — the relay entry points of libdrp (include/drp.h): drp_select_device and
// drp_latest_device over the caller's decoded columns, drp_relay_staged and drp_latest_staged over
// the batch last staged (select or latest per key, then the encoder with the staged wire as its
// heap), drp_fanout_device / drp_fanout_staged (many filters over one pass) and
// drp_fanout_latest_device / drp_fanout_latest_staged (latest per key under each), and the store
// (drp_store_*: the latest-per-key step, then the merge into caller-owned device memory; with a
// report, drp_store_merge_report_device, drp_store_merge_news_staged / drp_fanout_news_staged; the
// read-only probe by key, drp_store_lookup_device / drp_store_lookup_staged; the load of rows known
// to be new and the table's rebuild, drp_store_load_device / drp_store_rehash_device), and the
// digest calls (drp_digest_device, drp_digest_diff_device, drp_select_buckets_device, and their second
// level drp_digest_refine_device, drp_digest_diff_cells_device, drp_select_refined_device), and the ordered
// catch-up (drp_order_device). The kernels are in drp_select.hip, drp_latest.hip, drp_fanout.hip,
// drp_store.hip, drp_digest.hip and drp_order.hip; the context is drp_api.hip's (drp_ctx.h).
#include <algorithm>
#include <cstring>

#include "drp_ctx.h"
#include "drp_kernels.h"

using namespace drp;

// the decoded columns and the caller's row arrays are all there (n > 0)
static bool cols_ok(const drp_frames *frames, const drp_changes *cols, uint64_t n) {
  return !n || (frames->payload_off && frames->type && cols->key_off && cols->key_len && cols->subset_off &&
                cols->subset_len && cols->value_off && cols->value_len && cols->change && cols->from && cols->to &&
                cols->flags);
}
static bool rows_ok(const drp_frames *frames, const drp_changes *cols, const drp_change_src *out_rows, uint64_t n) {
  return !n || (cols_ok(frames, cols, n) && out_rows->key_off && out_rows->key_len && out_rows->subset_off &&
                out_rows->subset_len && out_rows->value_off && out_rows->value_len && out_rows->change &&
                out_rows->from && out_rows->to && out_rows->flags);
}

static bool src_cols_ok(const drp_change_src *r) {
  return r->key_off && r->key_len && r->subset_off && r->subset_len && r->value_off && r->value_len && r->change &&
         r->from && r->to && r->flags;
}

// drp_filter -> the kernels' filter record and its byte strings (fb: FAN_FBYTES bytes, zeroed by the
// caller). DRP_E_INVAL: unknown bits, EQ together with NONE, a string longer than
// DRP_SEL_MAX_BYTES or missing
static int select_filter(const drp_filter *f, RowFilter &F, uint8_t *fb) {
  F = RowFilter{0, 0, 0, 0, 0, ~0ull};
  if (!f) return DRP_OK;
  if (f->flags & ~drp_select_known_flags()) return DRP_E_INVAL;
  if ((f->flags & DRP_SEL_SUBSET_EQ) && (f->flags & DRP_SEL_SUBSET_NONE)) return DRP_E_INVAL;
  F.flags = f->flags;
  if (f->flags & DRP_SEL_CHANGE_RANGE) {
    F.change_min = f->change_min;
    F.change_max = f->change_max;
  }
  if (f->flags & DRP_SEL_SUBSET_EQ) {
    if (f->subset_len > DRP_SEL_MAX_BYTES || (f->subset_len && !f->subset)) return DRP_E_INVAL;
    F.subset_len = f->subset_len;
    if (f->subset_len) memcpy(fb, f->subset, f->subset_len);
  }
  if (f->flags & DRP_SEL_KEY_PREFIX) {
    if (f->key_prefix_len > DRP_SEL_MAX_BYTES || (f->key_prefix_len && !f->key_prefix)) return DRP_E_INVAL;
    F.prefix_len = f->key_prefix_len;
    if (f->key_prefix_len) memcpy(fb + DRP_SEL_MAX_BYTES, f->key_prefix, f->key_prefix_len);
  }
  return DRP_OK;
}

// the caller's decoded columns as the kernels' row source
static RowSrc caller_src(const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames, const drp_changes *cols,
                         uint64_t n) {
  RowSrc R = {};
  R.bytes = bytes;
  R.nbytes = nbytes;
  R.payload_off = frames->payload_off;
  R.type = frames->type;
  R.cols = *cols;
  R.n = n;
  return R;
}

// the staged batch's delivered GPU rows as the kernels' row source. A piece's payload offsets are
// relative to the batch offset it was staged at, and the staged bytes start at batch offset S.base
// (a leading blob continuation never reaches the device): the table of several pieces goes to
// piece_dev (2 * pieces words of device memory) through c->host_tmp
static int staged_src(drp_ctx *c, RowSrc &R, uint64_t *piece_dev) {
  const auto &S = c->staged;
  const uint64_t np = S.pieces.size();
  R = caller_src(S.wire, S.wire_bytes, &S.fr, &S.co, S.good);
  if (np > 1) {
    std::vector<uint64_t> &h = c->host_tmp;
    h.resize(2 * np);
    for (uint64_t k = 0; k < np; k++) {
      h[k] = S.pieces[k].first;
      h[np + k] = S.pieces[k].second - S.base;
    }
    CHK(hipMemcpyAsync(piece_dev, h.data(), 2 * np * 8, hipMemcpyHostToDevice, c->st));
    R.piece_row = piece_dev;
    R.piece_shift = piece_dev + np;
    R.npieces = np;
  } else {
    R.shift0 = np ? S.pieces[0].second - S.base : 0;
  }
  return DRP_OK;
}

// ten row columns of `stride` bytes each out of buf, from byte o on
static drp_change_src carve_rows(const DevBuf &buf, size_t o, size_t stride) {
  auto take = [&]() { void *p = buf.at<char>(o); o += stride; return p; };
  drp_change_src r;
  r.key_off = (const uint64_t *)take();
  r.key_len = (const uint32_t *)take();
  r.subset_off = (const uint64_t *)take();
  r.subset_len = (const uint32_t *)take();
  r.value_off = (const uint64_t *)take();
  r.value_len = (const uint32_t *)take();
  r.change = (const uint64_t *)take();
  r.from = (const uint64_t *)take();
  r.to = (const uint64_t *)take();
  r.flags = (const uint8_t *)take();
  return r;
}

// (the row arrays are writable device memory behind drp_change_src's const pointers)
static RowOut row_out(const drp_change_src *o, uint64_t *sel_idx) {
  RowOut r;
  r.o_key_off = const_cast<uint64_t *>(o->key_off);
  r.o_key_len = const_cast<uint32_t *>(o->key_len);
  r.o_subset_off = const_cast<uint64_t *>(o->subset_off);
  r.o_subset_len = const_cast<uint32_t *>(o->subset_len);
  r.o_value_off = const_cast<uint64_t *>(o->value_off);
  r.o_value_len = const_cast<uint32_t *>(o->value_len);
  r.o_change = const_cast<uint64_t *>(o->change);
  r.o_from = const_cast<uint64_t *>(o->from);
  r.o_to = const_cast<uint64_t *>(o->to);
  r.o_flags = const_cast<uint8_t *>(o->flags);
  r.sel_idx = sel_idx;
  return r;
}

static uint64_t select_scratch(uint64_t n, bool latest) {
  return latest ? drp_latest_scratch_bytes(n) : drp_select_scratch_bytes(n);
}

static hipError_t launch_select(drp_ctx *c, const SelectParams &P, const SelectBytes &fb, bool latest) {
  return latest ? drp_launch_latest(&P, &fb, c->latest_hash_mask, c->scratch.p, c->st)
                : drp_launch_select(&P, &fb, c->scratch.p, c->st);
}

// drp_select_device, or with `latest` drp_latest_device: the same arguments and checks
static int select_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                         const drp_changes *cols, uint64_t n, const drp_filter *filter, const drp_change_src *out_rows,
                         uint64_t *sel_idx, uint64_t *n_selected, bool latest) {
  if (!c || !frames || !cols || !out_rows || !n_selected || (!bytes && nbytes)) return DRP_E_INVAL;
  if (!rows_ok(frames, cols, out_rows, n)) return DRP_E_INVAL;
  SelectParams P = {};
  SelectBytes fb = {};
  if (const int rc = select_filter(filter, P.f, fb.b)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  // (the decode scratch: free between decodes, and every user is ordered on the ctx's stream)
  if (!c->scratch.ensure(select_scratch(n, latest))) return DRP_E_NOMEM;
  P.src = caller_src(bytes, nbytes, frames, cols, n);
  P.out = row_out(out_rows, sel_idx);
  P.n_selected = n_selected;
  CHK(launch_select(c, P, fb, latest));
  return DRP_OK;
}

// drp_relay_staged, or with `latest` drp_latest_staged: the latest-per-key step in the select's place
static int relay_staged(drp_ctx *c, const drp_filter *filter, uint8_t *out, uint64_t cap, uint64_t *written,
                        uint64_t *n_selected, bool latest) {
  if (!c || !written || !n_selected || (!out && cap)) return DRP_E_INVAL;
  const auto &S = c->staged;
  if (!S.valid) return DRP_E_INVAL;
  SelectParams P = {};
  SelectBytes fb = {};
  if (const int rc = select_filter(filter, P.f, fb.b)) return rc;
  *written = 0;
  *n_selected = 0;
  const uint64_t n = S.good;  // the delivered GPU rows (a carried blob's row 0 is built on the host)
  if (!n) return DRP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  // scratch (the decode's, free until the next decode): the kernel's words, the count, the piece
  // table, the selected rows' columns
  const size_t o_cnt = al(select_scratch(n, latest)), o_piece = o_cnt + 256,
               o_rows = o_piece + al(2 * S.pieces.size() * 8), col = al(n * 8);
  if (!c->scratch.ensure(o_rows + 10 * col)) return DRP_E_NOMEM;
  uint64_t *dcnt = c->scratch.at<uint64_t>(o_cnt);
  const drp_change_src rows = carve_rows(c->scratch, o_rows, col);
  if (const int rc = staged_src(c, P.src, c->scratch.at<uint64_t>(o_piece))) return rc;
  P.out = row_out(&rows, nullptr);
  P.n_selected = dcnt;
  CHK(launch_select(c, P, fb, latest));
  uint64_t nsel = 0;
  CHK(hipMemcpyAsync(&nsel, dcnt, 8, hipMemcpyDeviceToHost, c->st));
  CHK(hipStreamSynchronize(c->st));  // (the one readback that sizes the encode)
  *n_selected = nsel;
  return drp_encode_batch(c, &rows, S.wire, S.wire_bytes, nsel, out, cap, written);
}

// ---- fan-out ------------------------------------------------------------------------------------
// The filters, checked as select_filter checks one, into c->host_tmp in the device table's layout:
// nfilters records, then every filter's byte strings at FAN_FBYTES steps. (Checked there first: a bad
// filter leaves the page-locked table alone.)
static size_t fanout_table_bytes(uint32_t K) { return al((size_t)K * sizeof(RowFilter)) + (size_t)K * FAN_FBYTES; }

static int fanout_filters(drp_ctx *c, const drp_filter *filters, uint32_t K, FanParams &P) {
  if (!filters || K == 0 || K > DRP_FANOUT_MAX) return DRP_E_INVAL;
  std::vector<uint64_t> &h = c->host_tmp;
  h.assign((fanout_table_bytes(K) + 7) / 8, 0);
  RowFilter *tab = reinterpret_cast<RowFilter *>(h.data());
  uint8_t *fbytes = reinterpret_cast<uint8_t *>(h.data()) + al((size_t)K * sizeof(RowFilter));
  P.nfilters = K;
  P.any_flags = P.any_bytes = 0;
  for (uint32_t f = 0; f < K; f++) {
    if (const int rc = select_filter(&filters[f], tab[f], fbytes + (size_t)f * FAN_FBYTES)) return rc;
    P.any_flags |= tab[f].flags;
    P.any_bytes |= filter_bytes(tab[f]);
  }
  return DRP_OK;
}

// (after the scratch is placed) the checked table of fanout_filters to the device. It travels by one
// asynchronous copy out of the ctx's page-locked table, so before that is rewritten the copy of the
// previous call must have read it.
static int fanout_send_filters(drp_ctx *c, const FanParams &P) {
  const size_t total = fanout_table_bytes(P.nfilters);
  if (!c->fan_ev && hipEventCreateWithFlags(&c->fan_ev, hipEventDisableTiming) != hipSuccess) return DRP_E_HIP;
  CHK(hipEventSynchronize(c->fan_ev));  // (never recorded: returns at once)
  if (!c->fan_tab.ensure(total)) return DRP_E_NOMEM;
  memcpy(c->fan_tab.p, c->host_tmp.data(), total);
  // (filt is the scratch's first byte and the byte strings follow at the same offset as in the table)
  CHK(hipMemcpyAsync(const_cast<RowFilter *>(P.filt), c->fan_tab.p, total, hipMemcpyHostToDevice, c->st));
  CHK(hipEventRecord(c->fan_ev, c->st));
  return DRP_OK;
}

// the fan-out's scratch and count step; with `latest` the planes are cut down to their latest row
// per key between the ballots and the scan (drp_latest.hip)
static uint32_t latest_pass(const drp_ctx *c) { return c->fanout_latest_pass ? c->fanout_latest_pass : FLAT_PASS_DEFAULT; }

static uint64_t fanout_scratch(const drp_ctx *c, uint64_t n, uint32_t K, bool latest) {
  return latest ? drp_fanout_latest_scratch_bytes(n, K, latest_pass(c)) : drp_fanout_scratch_bytes(n, K);
}

static hipError_t launch_fanout_count(drp_ctx *c, const FanParams &P, bool latest) {
  if (!latest) return drp_launch_fanout_count(&P, c->st);
  if (const hipError_t e = drp_launch_fanout_ballot(&P, c->st)) return e;
  if (const hipError_t e = drp_launch_fanout_latest(&P, c->latest_hash_mask, latest_pass(c), c->scratch.p, c->st))
    return e;
  return drp_launch_fanout_scan(&P, c->st);
}

// drp_fanout_device, or with `latest` drp_fanout_latest_device (splice NULL)
static int fanout_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                         const drp_changes *cols, uint64_t n, const drp_filter *filters, uint32_t nfilters,
                         const drp_change_src *out_rows, uint64_t rows_cap, uint64_t *sel_idx, uint64_t *row_base,
                         const drp_splice *splice, bool latest) {
  if (!c || !frames || !cols || !out_rows || !row_base || (!bytes && nbytes)) return DRP_E_INVAL;
  if (!rows_ok(frames, cols, out_rows, n)) return DRP_E_INVAL;
  if (splice && (!splice->n_blobs || (splice->blob_cap && (!splice->blob_row || !splice->blob_rank)))) return DRP_E_INVAL;
  FanParams P = {};
  if (const int rc = fanout_filters(c, filters, nfilters, P)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  // (the decode scratch: free between decodes, and every user is ordered on the ctx's stream)
  if (!c->scratch.ensure(fanout_scratch(c, n, nfilters, latest))) return DRP_E_NOMEM;
  P.src = caller_src(bytes, nbytes, frames, cols, n);
  drp_fanout_place(&P, c->scratch.p);
  P.out = row_out(out_rows, sel_idx);
  P.rows_cap = rows_cap;
  P.row_base = row_base;
  if (const int rc = fanout_send_filters(c, P)) return rc;
  CHK(launch_fanout_count(c, P, latest));
  CHK(drp_launch_fanout_scatter(&P, c->st));
  if (splice) {
    P.blob_row = splice->blob_row;
    P.blob_rank = splice->blob_rank;
    P.n_blobs = splice->n_blobs;
    P.blob_cap = splice->blob_cap;
    CHK(drp_launch_fanout_splice(&P, c->st));
  }
  return DRP_OK;
}

// drp_fanout_staged, or with `latest` drp_fanout_latest_staged (no splice table: blob_row NULL), or
// with `news` drp_fanout_news_staged: the column drp_store_merge_news_staged kept in the staged type
// column's place
static int fanout_staged(drp_ctx *c, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                         uint64_t *out_off, uint64_t *n_selected, uint64_t *blob_row, uint64_t *blob_pos,
                         uint64_t blob_cap, uint64_t *n_blobs, bool latest, bool news = false) {
  if (!c || !out_off || !n_selected || (!out && cap)) return DRP_E_INVAL;
  if (blob_row ? (!n_blobs || (!blob_pos && blob_cap)) : (n_blobs != nullptr)) return DRP_E_INVAL;
  const auto &S = c->staged;
  if (!S.valid) return DRP_E_INVAL;
  if (news && !(c->news_held && c->news_seq == S.seq)) return DRP_E_INVAL;
  FanParams P = {};
  if (const int rc = fanout_filters(c, filters, nfilters, P)) return rc;
  const uint32_t K = nfilters;
  for (uint32_t f = 0; f <= K; f++) out_off[f] = 0;
  for (uint32_t f = 0; f < K; f++) n_selected[f] = 0;
  if (n_blobs) *n_blobs = 0;
  const uint64_t n = S.good;  // the delivered GPU rows (a carried blob's row 0 is built on the host)
  if (!n) return DRP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  hipStream_t st = c->st;
  // scratch (the decode's, free until the next decode): the kernels' words, row_base with the grand
  // total and the splice kernel's blob count behind it, the piece table
  const size_t o_base = al(fanout_scratch(c, n, K, latest)), o_piece = o_base + al((K + 3) * 8);
  if (!c->scratch.ensure(o_piece + al(2 * S.pieces.size() * 8))) return DRP_E_NOMEM;
  P.src.n = n;
  drp_fanout_place(&P, c->scratch.p);
  uint64_t *drb = c->scratch.at<uint64_t>(o_base);
  P.row_base = drb;
  P.gtotal = drb + K + 1;  // (one readback brings the outputs' bounds and the blob count)
  if (const int rc = fanout_send_filters(c, P)) return rc;
  // (c->host_tmp's filter table has been copied out: the piece table may pass through it)
  if (const int rc = staged_src(c, P.src, c->scratch.at<uint64_t>(o_piece))) return rc;
  if (news) P.src.type = c->news.at<uint8_t>(0);
  CHK(launch_fanout_count(c, P, latest));
  uint64_t rb[DRP_FANOUT_MAX + 2];
  CHK(hipMemcpyAsync(rb, drb, (K + 2) * 8, hipMemcpyDeviceToHost, st));
  CHK(hipStreamSynchronize(st));  // (the one readback that sizes the rows and the encode)
  const uint64_t total = rb[K], nb_true = rb[K + 1] - rb[K];
  for (uint32_t f = 0; f < K; f++) n_selected[f] = rb[f + 1] - rb[f];
  if (n_blobs) *n_blobs = nb_true;
  const uint64_t nb = (blob_row && nb_true <= blob_cap) ? nb_true : 0;  // the splice entries to produce
  // the selected rows (sized from the true total) and the splice kernel's outputs
  const size_t col = al(total * 8), o_brow = 10 * col, o_rank = o_brow + al(nb * 8);
  if (!c->fan_rows.ensure(o_rank + al((size_t)K * nb * 8) + 256)) return DRP_E_NOMEM;
  const drp_change_src rows = carve_rows(c->fan_rows, 0, col);
  P.out = row_out(&rows, nullptr);
  P.rows_cap = total;
  CHK(drp_launch_fanout_scatter(&P, st));
  uint64_t *drank = c->fan_rows.at<uint64_t>(o_rank);
  if (nb) {
    P.blob_row = c->fan_rows.at<uint64_t>(o_brow);
    P.blob_rank = drank;
    P.n_blobs = drb + K + 2;  // (a word of its own: the grand total is still read by the kernel)
    P.blob_cap = nb;
    P.row_bias = S.nf0;
    CHK(drp_launch_fanout_splice(&P, st));
  }
  // one encode of all outputs; its bytes go to `out` or, for a host `out`, to the output staging,
  // which need not be larger than the outputs can get (none is longer than the staged wire)
  const bool odev = is_device_ptr(out);
  uint64_t nonempty = 0;
  for (uint32_t f = 0; f < K; f++) nonempty += n_selected[f] != 0;
  const uint64_t dcap = odev ? cap : std::min<uint64_t>(cap, nonempty * S.wire_bytes);
  const size_t o_gat = al((total + 1) * 8), gat_n = (size_t)K + 1 + (size_t)K * nb, o_out = o_gat + al(gat_n * 8);
  if (!c->out_stage.ensure(o_out + (odev ? 0 : dcap + 64))) return DRP_E_NOMEM;
  uint64_t *foff = c->out_stage.at<uint64_t>(0), *dgat = c->out_stage.at<uint64_t>(o_gat);
  uint8_t *dout = odev ? out : c->out_stage.at<uint8_t>(o_out);
  if (const int rc = drp_encode_device(c, &rows, S.wire, S.wire_bytes, total, foff, dout, dcap)) return rc;
  // the outputs' bounds and the blobs' byte positions, gathered into one block for one readback
  CHK(drp_launch_fanout_gather(foff, drb, K, drank, nb, dgat, dgat + K + 1, st));
  std::vector<uint64_t> &h = c->host_tmp;
  h.resize(gat_n + nb);
  CHK(hipMemcpyAsync(h.data(), dgat, gat_n * 8, hipMemcpyDeviceToHost, st));
  if (nb) CHK(hipMemcpyAsync(h.data() + gat_n, P.blob_row, nb * 8, hipMemcpyDeviceToHost, st));
  CHK(hipStreamSynchronize(st));
  if (h[K] == ~0ull) return DRP_E_INVAL;  // a row's key/subset/value range is outside the wire
  for (uint32_t f = 0; f <= K; f++) out_off[f] = h[f];
  if (h[K] > cap) return DRP_E_CAPACITY;
  for (uint64_t j = 0; j < nb; j++) blob_row[j] = h[gat_n + j];
  for (uint32_t f = 0; f < K && nb; f++)
    memcpy(blob_pos + (uint64_t)f * blob_cap, h.data() + K + 1 + (uint64_t)f * nb, nb * 8);
  if (!odev && h[K]) {
    CHK(hipMemcpyAsync(out, dout, h[K], hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
  }
  return DRP_OK;
}

// ---- store --------------------------------------------------------------------------------------
// the caller's drp_store as the kernels take it; false: a NULL pointer, a misaligned arena,
// max_keys out of range
static bool store_dev(const drp_ctx *c, const drp_store *s, StoreDev &D) {
  const drp_changes &co = s->cols;
  D.nslots = drp_store_nslots(s->max_keys);
  if (!D.nslots || !s->table || !s->info || (!s->arena && s->arena_bytes) || ((uintptr_t)s->arena & 15)) return false;
  if (!s->frames.payload_off || !s->frames.payload_len || !s->frames.type || !co.key_off || !co.key_len ||
      !co.subset_off || !co.subset_len || !co.value_off || !co.value_len || !co.change || !co.from || !co.to ||
      !co.flags)
    return false;
  D.arena = s->arena;
  D.arena_bytes = s->arena_bytes;
  D.payload_off = s->frames.payload_off;
  D.payload_len = s->frames.payload_len;
  D.type = s->frames.type;
  D.cols = co;
  D.max_keys = s->max_keys;
  D.table = s->table;
  D.hash_mask = c->latest_hash_mask;
  D.info = s->info;
  return true;
}

// A merge of the rows `src` describes (the caller's, or the staged batch's when `staged`): the
// latest-per-key step into winner rows in the ctx's scratch, then drp_store.hip's steps over them.
// Scratch: drp_launch_latest's words, the winners' count, the staged piece table, the winner rows
// (ten columns of n entries), the merge's state; behind it, only when the report `rep` (NULL: none)
// asks for them, the winners' source rows and the workgroups' stale counts.
// With `load` the load of include/drp.h "store lifecycle" (no report): the plain select in the
// latest's place, with its smaller scratch, and drp_launch_store_load over its rows
static int store_merge(drp_ctx *c, const StoreDev &D, const RowSrc *caller, const drp_filter *filter,
                       const drp_merge_report *rep = nullptr, bool load = false, uint64_t *clash = nullptr) {
  SelectParams P = {};
  SelectBytes fb = {};
  if (const int rc = select_filter(filter, P.f, fb.b)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  const auto &S = c->staged;
  const uint64_t n = caller ? caller->n : S.good, np = caller ? 0 : S.pieces.size();
  const bool by_row = rep && (rep->outcome || rep->news_type), reply = rep && rep->n_reply;
  const size_t o_cnt = al(select_scratch(n, !load)), o_piece = o_cnt + 256, o_rows = o_piece + al(2 * np * 8),
               col = al(n * 8), o_state = o_rows + 10 * col, o_src = o_state + drp_store_merge_scratch_bytes(n),
               o_stale = o_src + (by_row ? col : 0), o_end = o_stale + (reply ? al(drp_store_blocks(n) * 8) : 0);
  if (!c->scratch.ensure(o_end)) return DRP_E_NOMEM;
  if (caller) P.src = *caller;
  else if (const int rc = staged_src(c, P.src, c->scratch.at<uint64_t>(o_piece))) return rc;
  const drp_change_src rows = carve_rows(c->scratch, o_rows, col);
  P.out = row_out(&rows, by_row ? c->scratch.at<uint64_t>(o_src) : nullptr);
  P.n_selected = c->scratch.at<uint64_t>(o_cnt);
  CHK(launch_select(c, P, fb, !load));
  StoreMerge M = {};
  M.s = D;
  M.bytes = P.src.bytes;
  M.nbytes = P.src.nbytes;
  M.w = rows;
  M.nw = P.n_selected;
  M.n = n;
  if (load) {
    CHK(drp_launch_store_load(&M, clash, c->scratch.at<char>(o_state), c->st));
    return DRP_OK;
  }
  StoreReport R = {};
  if (by_row || reply) {
    R.flags = rep->flags;
    R.type = P.src.type;
    R.outcome = rep->outcome;
    R.news_type = rep->news_type;
    R.src_row = P.out.sel_idx;
    if (rep->reply_rows && rep->reply_cap) R.reply = row_out(rep->reply_rows, rep->reply_idx);
    R.n_reply = rep->n_reply;
    R.reply_cap = rep->reply_rows ? rep->reply_cap : 0;
    R.blk_stale = reply ? c->scratch.at<uint64_t>(o_stale) : nullptr;
  }
  CHK(drp_launch_store_merge(&M, (by_row || reply) ? &R : nullptr, c->scratch.at<char>(o_state), c->st));
  return DRP_OK;
}

// the report's own DRP_E_INVAL cases (type: the batch's type column)
static bool report_ok(const drp_merge_report *rep, const uint8_t *type) {
  if (!rep) return true;
  if (rep->flags & ~(uint32_t)DRP_REPORT_KEEP_BLOBS) return false;
  if (rep->reply_rows && (!rep->n_reply || (rep->reply_cap && !src_cols_ok(rep->reply_rows)))) return false;
  return !(rep->news_type && rep->news_type == type);
}

// ---- lookup -------------------------------------------------------------------------------------
constexpr uint32_t LOOKUP_EMIT_BITS =
    DRP_LOOKUP_BIT(DRP_LOOKUP_BEHIND) | DRP_LOOKUP_BIT(DRP_LOOKUP_LEVEL) | DRP_LOOKUP_BIT(DRP_LOOKUP_AHEAD);

// the DRP_E_INVAL cases of a drp_lookup that need neither the ctx nor a device (type: the store's
// type column)
static bool lookup_ok(const drp_lookup *lk, const uint8_t *type) {
  if (!lk || lk->flags || (lk->emit_mask & ~LOOKUP_EMIT_BITS)) return false;
  if (lk->out_rows && (!lk->n_out || (lk->rows_cap && !src_cols_ok(lk->out_rows)))) return false;
  return !(lk->lack_type && lk->lack_type == type);
}

// The lookup of the rows of `src` under the filter F / fb against D, its state `at` bytes into the
// ctx's scratch (ensured by the caller: drp_store_lookup_scratch_bytes(src.n) bytes from there)
static int store_lookup(drp_ctx *c, const StoreDev &D, const RowSrc &src, const RowFilter &F, const SelectBytes &fb,
                        const drp_lookup *lk, size_t at) {
  StoreLookup Q = {};
  Q.s = D;
  Q.sel.src = src;
  Q.sel.f = F;
  Q.emit_mask = lk->emit_mask;  // (n_out without out_rows: the count alone, as with rows_cap 0)
  Q.verdict = lk->verdict;
  Q.hit_row = lk->hit_row;
  Q.counts = lk->counts;
  Q.lack_type = lk->lack_type;
  if (lk->out_rows && lk->rows_cap) Q.out = row_out(lk->out_rows, lk->out_query);
  Q.n_out = lk->n_out;
  Q.rows_cap = lk->out_rows ? lk->rows_cap : 0;
  CHK(drp_launch_store_lookup(&Q, &fb, c->scratch.at<char>(at), c->st));
  return DRP_OK;
}

static int store_query(drp_ctx *c, const drp_store_info *dev, drp_store_info *host) {
  CHK(hipMemcpyAsync(host, dev, sizeof(drp_store_info), hipMemcpyDeviceToHost, c->st));
  CHK(hipStreamSynchronize(c->st));
  return DRP_OK;
}

// ---- digest / reconcile ---------------------------------------------------------------------------
// the arguments drp_digest_device and drp_select_buckets_device share, into D (out_rows NULL: the
// digest, which writes no rows)
static int digest_params(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                         const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                         const drp_change_src *out_rows, DigestParams &D, SelectBytes &fb) {
  if (!c || !frames || !cols || (!bytes && nbytes) || bits > DRP_DIGEST_MAX_BITS) return DRP_E_INVAL;
  if (out_rows ? !rows_ok(frames, cols, out_rows, n) : !cols_ok(frames, cols, n)) return DRP_E_INVAL;
  if (const int rc = select_filter(filter, D.sel.f, fb.b)) return rc;
  D.sel.src = caller_src(bytes, nbytes, frames, cols, n);
  D.bits = bits;
  return DRP_OK;
}

extern "C" {

int drp_digest_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                      drp_digest_cell *cells, uint64_t *totals) {
  DigestParams D = {};
  SelectBytes fb = {};
  if (!cells) return DRP_E_INVAL;
  if (const int rc = digest_params(c, bytes, nbytes, frames, cols, n, filter, bits, nullptr, D, fb)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  if (!c->scratch.ensure(2 * DRP_SEL_MAX_BYTES)) return DRP_E_NOMEM;
  D.cells = cells;
  D.totals = totals;
  CHK(drp_launch_digest(&D, &fb, c->scratch.p, c->st));
  return DRP_OK;
}

int drp_digest_diff_device(drp_ctx *c, const drp_digest_cell *a, const drp_digest_cell *b, uint32_t bits,
                           uint64_t *bucket_set, uint64_t *n_diff) {
  if (!c || !a || !b || !bucket_set || !n_diff || bits > DRP_DIGEST_MAX_BITS) return DRP_E_INVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  CHK(drp_launch_digest_diff(a, b, bits, bucket_set, n_diff, c->st));
  return DRP_OK;
}

int drp_select_buckets_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                              const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                              const uint64_t *bucket_set, const drp_change_src *out_rows, uint64_t *sel_idx,
                              uint64_t *n_selected) {
  DigestParams D = {};
  SelectBytes fb = {};
  if (!bucket_set || !out_rows || !n_selected) return DRP_E_INVAL;
  if (const int rc = digest_params(c, bytes, nbytes, frames, cols, n, filter, bits, out_rows, D, fb)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  if (!c->scratch.ensure(drp_select_scratch_bytes(n))) return DRP_E_NOMEM;
  D.bucket_set = bucket_set;
  D.sel.out = row_out(out_rows, sel_idx);
  D.sel.n_selected = n_selected;
  CHK(drp_launch_select_buckets(&D, &fb, c->scratch.p, c->st));
  return DRP_OK;
}

// the second level: the set, sub_bits and the rank table's place (`rank_at` bytes into the scratch)
static void refine_params(drp_ctx *c, RefineParams &R, const uint64_t *bucket_set, uint32_t sub_bits, size_t rank_at) {
  R.d.bucket_set = bucket_set;
  R.sub_bits = sub_bits;
  R.set_words = std::max(1u, (1u << R.d.bits) / 64);
  R.rank = c->scratch.at<uint32_t>(rank_at);
}
static bool sub_bits_ok(uint32_t sub_bits) { return sub_bits >= 1 && sub_bits <= DRP_DIGEST_MAX_SUB_BITS; }

int drp_digest_refine_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                             const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                             const uint64_t *bucket_set, uint32_t sub_bits, drp_digest_cell *cells2,
                             uint64_t cells_cap, uint64_t *totals) {
  RefineParams R = {};
  SelectBytes fb = {};
  if (!bucket_set || !cells2 || !totals || !sub_bits_ok(sub_bits)) return DRP_E_INVAL;
  if (const int rc = digest_params(c, bytes, nbytes, frames, cols, n, filter, bits, nullptr, R.d, fb)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  const size_t rank_at = 2 * DRP_SEL_MAX_BYTES;
  if (!c->scratch.ensure(rank_at + 4 * DIG_RANK_BLK)) return DRP_E_NOMEM;
  refine_params(c, R, bucket_set, sub_bits, rank_at);
  R.d.cells = cells2;
  R.d.totals = totals;
  R.cells_cap = cells_cap;
  CHK(drp_launch_digest_refine(&R, &fb, c->scratch.p, c->st));
  return DRP_OK;
}

int drp_digest_diff_cells_device(drp_ctx *c, const drp_digest_cell *a, const drp_digest_cell *b, uint64_t ncells,
                                 uint64_t *cell_set, uint64_t *n_diff) {
  const uint64_t most = (uint64_t)1 << (DRP_DIGEST_MAX_BITS + DRP_DIGEST_MAX_SUB_BITS);
  if (!c || !a || !b || !cell_set || !n_diff || ncells > most) return DRP_E_INVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  CHK(drp_launch_digest_diff_cells(a, b, (uint32_t)ncells, cell_set, n_diff, c->st));
  return DRP_OK;
}

int drp_select_refined_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                              const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                              const uint64_t *bucket_set, uint32_t sub_bits, const uint64_t *cell_set,
                              const drp_change_src *out_rows, uint64_t *sel_idx, uint64_t *n_selected) {
  RefineParams R = {};
  SelectBytes fb = {};
  if (!bucket_set || !cell_set || !out_rows || !n_selected || !sub_bits_ok(sub_bits)) return DRP_E_INVAL;
  if (const int rc = digest_params(c, bytes, nbytes, frames, cols, n, filter, bits, out_rows, R.d, fb)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  const size_t rank_at = (drp_select_scratch_bytes(n) + 7) & ~(size_t)7;
  if (!c->scratch.ensure(rank_at + 4 * DIG_RANK_BLK)) return DRP_E_NOMEM;
  refine_params(c, R, bucket_set, sub_bits, rank_at);
  R.cell_set = cell_set;
  R.d.sel.out = row_out(out_rows, sel_idx);
  R.d.sel.n_selected = n_selected;
  CHK(drp_launch_select_refined(&R, &fb, c->scratch.p, c->st));
  return DRP_OK;
}

// ---- ordered catch-up ---------------------------------------------------------------------------
int drp_order_device(drp_ctx *c, const drp_change_src *rows, const uint64_t *row_base, uint32_t nseg,
                     uint64_t rows_cap, const uint64_t *limit, uint32_t flags, const drp_change_src *out_rows,
                     const uint64_t *sel_idx, uint64_t *out_sel_idx, uint64_t *out_base) {
  if (!c || !rows || !row_base || !out_rows || !out_base || nseg == 0 || nseg > DRP_FANOUT_MAX) return DRP_E_INVAL;
  if ((flags & ~(uint32_t)DRP_ORDER_KEEP_TIES) || (out_sel_idx && !sel_idx) || rows_cap > 0xFFFFFFFFull)
    return DRP_E_INVAL;
  if (rows_cap && (!src_cols_ok(rows) || !src_cols_ok(out_rows))) return DRP_E_INVAL;
  if (out_rows->change && out_rows->change == rows->change) return DRP_E_INVAL;  // (no in-place sort)
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  // (the decode scratch: free between decodes, and every user is ordered on the ctx's stream)
  if (!c->scratch.ensure(drp_order_scratch_bytes(rows_cap))) return DRP_E_NOMEM;
  OrderParams P = {};
  OrdLimits L;
  uint64_t out_max = 0;
  for (uint32_t f = 0; f < DRP_FANOUT_MAX; f++) {
    L.v[f] = limit && f < nseg ? limit[f] : ~0ull;
    if (f < nseg) out_max = out_max + L.v[f] < out_max ? ~0ull : out_max + L.v[f];
  }
  P.rows = *rows;
  P.row_base = row_base;
  P.nseg = nseg;
  P.flags = flags;
  P.rows_cap = rows_cap;
  P.out = row_out(out_rows, out_sel_idx);
  P.sel_idx = sel_idx;
  P.out_base = out_base;
  P.skip = c->order_skip ? 1 : 0;
  if (flags & DRP_ORDER_KEEP_TIES) out_max = ~0ull;  // (a cut that moves to its run's end passes the limit)
  CHK(drp_launch_order(&P, &L, out_max, c->scratch.p, c->st));
  return DRP_OK;
}

// ---- key-ordered listing ------------------------------------------------------------------------
int drp_order_keys_device(drp_ctx *c, const uint8_t *heap, uint64_t heap_bytes, const drp_change_src *rows,
                          const uint64_t *row_base, uint32_t nseg, uint64_t rows_cap, const drp_key_page *pages,
                          uint32_t flags, const drp_change_src *out_rows, const uint64_t *sel_idx,
                          uint64_t *out_sel_idx, uint64_t *out_base, uint64_t *totals) {
  if (!c || !rows || !row_base || !out_rows || !out_base || nseg == 0 || nseg > DRP_FANOUT_MAX) return DRP_E_INVAL;
  if ((flags & ~(uint32_t)DRP_KEYORDER_KEEP_TIES) || (out_sel_idx && !sel_idx) || rows_cap > 0xFFFFFFFFull)
    return DRP_E_INVAL;
  if (rows_cap && (!src_cols_ok(rows) || !src_cols_ok(out_rows))) return DRP_E_INVAL;
  if (out_rows->change && out_rows->change == rows->change) return DRP_E_INVAL;  // (no in-place sort)
  if (!heap && heap_bytes) return DRP_E_INVAL;
  const uint32_t page_bits = DRP_KEYPAGE_FROM | DRP_KEYPAGE_AFTER | DRP_KEYPAGE_UNTIL;
  OrdkPages G = {};
  uint64_t out_max = 0, nbound = 0;
  for (uint32_t f = 0; f < DRP_FANOUT_MAX; f++) {
    G.limit[f] = ~0ull;
    if (!pages || f >= nseg) continue;
    const drp_key_page &pg = pages[f];
    if ((pg.flags & ~page_bits) || ((pg.flags & DRP_KEYPAGE_FROM) && (pg.flags & DRP_KEYPAGE_AFTER))) return DRP_E_INVAL;
    if (pg.lo_len > DRP_KEYORDER_MAX_BYTES || pg.hi_len > DRP_KEYORDER_MAX_BYTES) return DRP_E_INVAL;
    if ((pg.lo_len && !pg.lo) || (pg.hi_len && !pg.hi)) return DRP_E_INVAL;
    G.limit[f] = pg.limit;
    G.flags[f] = pg.flags;
    if (pg.flags & (DRP_KEYPAGE_FROM | DRP_KEYPAGE_AFTER)) {
      G.lo_off[f] = (uint32_t)nbound;
      G.lo_len[f] = pg.lo_len;
      nbound += pg.lo_len;
    }
    if (pg.flags & DRP_KEYPAGE_UNTIL) {
      G.hi_off[f] = (uint32_t)nbound;
      G.hi_len[f] = pg.hi_len;
      nbound += pg.hi_len;
    }
  }
  for (uint32_t f = 0; f < nseg; f++) out_max = out_max + G.limit[f] < out_max ? ~0ull : out_max + G.limit[f];
  if (flags & DRP_KEYORDER_KEEP_TIES) out_max = ~0ull;  // (a cut that moves to its run's end passes the limit)
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  std::vector<uint8_t> bounds(nbound);  // (the bounds in use, end to end; copied before the call's one wait ends)
  for (uint32_t f = 0; pages && f < nseg; f++) {
    if (G.lo_len[f]) memcpy(bounds.data() + G.lo_off[f], pages[f].lo, G.lo_len[f]);
    if (G.hi_len[f]) memcpy(bounds.data() + G.hi_off[f], pages[f].hi, G.hi_len[f]);
  }
  // (the decode scratch: free between decodes, and every user is ordered on the ctx's stream)
  if (!c->scratch.ensure(drp_keyorder_scratch_bytes(rows_cap, nbound))) return DRP_E_NOMEM;
  KeyOrderParams K = {};
  OrderParams &P = K.o;
  P.rows = *rows;
  P.row_base = row_base;
  P.nseg = nseg;
  P.flags = flags;
  P.rows_cap = rows_cap;
  P.out = row_out(out_rows, out_sel_idx);
  P.sel_idx = sel_idx;
  P.out_base = out_base;
  P.skip = c->order_skip ? 1 : 0;
  K.heap = heap;
  K.heap_bytes = heap_bytes;
  K.bounds_bytes = nbound;
  K.totals = totals;
  CHK(drp_launch_keyorder(&K, &G, bounds.data(), out_max, c->scratch.p, c->st));
  return DRP_OK;
}

uint64_t drp_store_table_bytes(uint64_t max_keys) { return 8 * drp_store_nslots(max_keys); }

int drp_store_init(drp_ctx *c, const drp_store *s) {
  StoreDev D = {};
  if (!c || !s || !store_dev(c, s, D)) return DRP_E_INVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  CHK(drp_launch_store_init(&D, c->st));
  return DRP_OK;
}

int drp_store_merge_device(drp_ctx *c, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                           const drp_frames *frames, const drp_changes *cols, uint64_t n, const drp_filter *filter) {
  StoreDev D = {};
  if (!c || !s || !frames || !cols || (!bytes && nbytes) || !store_dev(c, s, D)) return DRP_E_INVAL;
  if (!cols_ok(frames, cols, n)) return DRP_E_INVAL;
  const RowSrc R = caller_src(bytes, nbytes, frames, cols, n);
  return store_merge(c, D, &R, filter);
}

int drp_store_merge_report_device(drp_ctx *c, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                                  const drp_frames *frames, const drp_changes *cols, uint64_t n,
                                  const drp_filter *filter, const drp_merge_report *report) {
  StoreDev D = {};
  if (!c || !s || !frames || !cols || (!bytes && nbytes) || !store_dev(c, s, D)) return DRP_E_INVAL;
  if (!cols_ok(frames, cols, n) || !report_ok(report, frames->type)) return DRP_E_INVAL;
  const RowSrc R = caller_src(bytes, nbytes, frames, cols, n);
  return store_merge(c, D, &R, filter, report);
}

int drp_store_load_device(drp_ctx *c, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                          const drp_frames *frames, const drp_changes *cols, uint64_t n, const drp_filter *filter,
                          uint64_t *clash) {
  StoreDev D = {};
  if (!c || !s || !frames || !cols || (!bytes && nbytes) || !store_dev(c, s, D)) return DRP_E_INVAL;
  if (!cols_ok(frames, cols, n)) return DRP_E_INVAL;
  const RowSrc R = caller_src(bytes, nbytes, frames, cols, n);
  return store_merge(c, D, &R, filter, nullptr, true, clash);
}

int drp_store_rehash_device(drp_ctx *c, const drp_store *s, uint64_t *report) {
  StoreDev D = {};
  if (!c || !s || !store_dev(c, s, D)) return DRP_E_INVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  CHK(drp_launch_store_rehash(&D, report, c->st));
  return DRP_OK;
}

// drp_store_merge_staged, or with `news` drp_store_merge_news_staged: the merge's news column, blobs
// kept, into c->news (a buffer of its own: the scratch is the next call's)
static int store_merge_staged(drp_ctx *c, const drp_store *s, const drp_filter *filter, drp_store_info *info_host,
                              bool news) {
  StoreDev D = {};
  if (!c || !s || !store_dev(c, s, D)) return DRP_E_INVAL;
  if (!c->staged.valid) return DRP_E_INVAL;
  drp_merge_report rep = {};
  if (news) {
    c->news_held = false;
    if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
    if (!c->news.ensure(c->staged.good + 16)) return DRP_E_NOMEM;
    rep.flags = DRP_REPORT_KEEP_BLOBS;
    rep.news_type = c->news.at<uint8_t>(0);
  }
  if (const int rc = store_merge(c, D, nullptr, filter, news ? &rep : nullptr)) return rc;
  drp_store_info I;
  if (const int rc = store_query(c, D.info, &I)) return rc;
  if (news) {  // (held after a refusal too: nothing is news then, and the blobs are still listed)
    c->news_held = true;
    c->news_seq = c->staged.seq;
  }
  if (info_host) *info_host = I;
  return I.refused ? DRP_E_CAPACITY : DRP_OK;
}

int drp_store_merge_staged(drp_ctx *c, const drp_store *s, const drp_filter *filter, drp_store_info *info_host) {
  return store_merge_staged(c, s, filter, info_host, false);
}

int drp_store_merge_news_staged(drp_ctx *c, const drp_store *s, const drp_filter *filter, drp_store_info *info_host) {
  return store_merge_staged(c, s, filter, info_host, true);
}

int drp_fanout_news_staged(drp_ctx *c, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                           uint64_t *out_off, uint64_t *n_selected, uint64_t *blob_row, uint64_t *blob_pos,
                           uint64_t blob_cap, uint64_t *n_blobs) {
  return fanout_staged(c, filters, nfilters, out, cap, out_off, n_selected, blob_row, blob_pos, blob_cap, n_blobs,
                       false, true);
}

int drp_store_lookup_device(drp_ctx *c, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                            const drp_frames *frames, const drp_changes *cols, uint64_t n, const drp_filter *filter,
                            const drp_lookup *lk) {
  StoreDev D = {};
  if (!c || !s || !frames || !cols || (!bytes && nbytes) || !lookup_ok(lk, s->frames.type)) return DRP_E_INVAL;
  if (!store_dev(c, s, D) || !cols_ok(frames, cols, n)) return DRP_E_INVAL;
  RowFilter F;
  SelectBytes fb = {};
  if (const int rc = select_filter(filter, F, fb.b)) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  // (the decode scratch: free between decodes, and every user is ordered on the ctx's stream)
  if (!c->scratch.ensure(drp_store_lookup_scratch_bytes(n))) return DRP_E_NOMEM;
  return store_lookup(c, D, caller_src(bytes, nbytes, frames, cols, n), F, fb, lk, 0);
}

// Scratch (the decode's, free until the next decode): with DRP_LOOKUP_REPLY_LACK the select's words
// for max_keys rows; the lookup's state; the counts (the reply's rows, then the five verdicts); the
// piece table; the reply's rows (ten columns of n entries, or of max_keys)
int drp_store_lookup_staged(drp_ctx *c, const drp_store *s, const drp_filter *filter, uint32_t reply, uint8_t *out,
                            uint64_t cap, uint64_t *written, uint64_t *n_rows, uint64_t *counts_host) {
  StoreDev D = {};
  const bool lack = reply == DRP_LOOKUP_REPLY_LACK;
  if (!c || !s || !written || !n_rows || (!out && cap) || (!lack && (reply & ~LOOKUP_EMIT_BITS))) return DRP_E_INVAL;
  if (!store_dev(c, s, D)) return DRP_E_INVAL;
  const auto &S = c->staged;
  if (!S.valid) return DRP_E_INVAL;
  RowFilter F;
  SelectBytes fb = {};
  if (const int rc = select_filter(filter, F, fb.b)) return rc;
  *written = 0;
  *n_rows = 0;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  const uint64_t n = S.good, cap_rows = lack ? D.max_keys : n;
  const size_t o_lk = lack ? al(drp_select_scratch_bytes(D.max_keys)) : 0,
               o_cnt = o_lk + al(drp_store_lookup_scratch_bytes(n)), o_piece = o_cnt + 256,
               o_rows = o_piece + al(2 * S.pieces.size() * 8), col = al(cap_rows * 8);
  if (!c->scratch.ensure(o_rows + 10 * col)) return DRP_E_NOMEM;
  if (lack && !c->lack.ensure(D.max_keys + 16)) return DRP_E_NOMEM;
  uint64_t *dcnt = c->scratch.at<uint64_t>(o_cnt);
  const drp_change_src rows = carve_rows(c->scratch, o_rows, col);
  RowSrc src;
  if (const int rc = staged_src(c, src, c->scratch.at<uint64_t>(o_piece))) return rc;
  drp_lookup lk = {};
  lk.counts = dcnt + 1;
  if (lack) {
    lk.lack_type = c->lack.at<uint8_t>(0);
  } else {
    lk.emit_mask = reply;
    lk.out_rows = &rows;
    lk.n_out = dcnt;
    lk.rows_cap = n;
  }
  if (const int rc = store_lookup(c, D, src, F, fb, &lk, o_lk)) return rc;
  if (lack) {  // the store's rows under lack_type, in store-row order
    SelectParams P = {};
    SelectBytes none = {};
    select_filter(nullptr, P.f, none.b);
    drp_frames fr = s->frames;
    fr.type = lk.lack_type;
    P.src = caller_src(D.arena, D.arena_bytes, &fr, &D.cols, D.max_keys);
    P.out = row_out(&rows, nullptr);
    P.n_selected = dcnt;
    CHK(drp_launch_select(&P, &none, c->scratch.p, c->st));
  }
  uint64_t h[1 + LK_CODES];
  CHK(hipMemcpyAsync(h, dcnt, sizeof h, hipMemcpyDeviceToHost, c->st));
  CHK(hipStreamSynchronize(c->st));  // (the one readback that sizes the encode)
  *n_rows = h[0];
  if (counts_host) memcpy(counts_host, h + 1, LK_CODES * 8);
  return drp_encode_batch(c, &rows, D.arena, D.arena_bytes, h[0], out, cap, written);
}

int drp_store_compact(drp_ctx *c, const drp_store *s, uint8_t *arena2, uint64_t arena2_bytes) {
  StoreDev D = {};
  if (!c || !s || !store_dev(c, s, D) || (!arena2 && arena2_bytes) || ((uintptr_t)arena2 & 15)) return DRP_E_INVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  if (!c->scratch.ensure(drp_store_compact_scratch_bytes(D.max_keys))) return DRP_E_NOMEM;
  CHK(drp_launch_store_compact(&D, arena2, arena2_bytes, c->scratch.p, c->st));
  return DRP_OK;
}

int drp_store_query(drp_ctx *c, const drp_store *s, drp_store_info *info_host) {
  if (!c || !s || !s->info || !info_host) return DRP_E_INVAL;
  if (hipSetDevice(c->device) != hipSuccess) return DRP_E_HIP;
  return store_query(c, s->info, info_host);
}

int drp_select_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filter, const drp_change_src *out_rows,
                      uint64_t *sel_idx, uint64_t *n_selected) {
  return select_device(c, bytes, nbytes, frames, cols, n, filter, out_rows, sel_idx, n_selected, false);
}

int drp_latest_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filter, const drp_change_src *out_rows,
                      uint64_t *sel_idx, uint64_t *n_selected) {
  return select_device(c, bytes, nbytes, frames, cols, n, filter, out_rows, sel_idx, n_selected, true);
}

int drp_relay_staged(drp_ctx *c, const drp_filter *filter, uint8_t *out, uint64_t cap, uint64_t *written,
                     uint64_t *n_selected) {
  return relay_staged(c, filter, out, cap, written, n_selected, false);
}

int drp_latest_staged(drp_ctx *c, const drp_filter *filter, uint8_t *out, uint64_t cap, uint64_t *written,
                      uint64_t *n_selected) {
  return relay_staged(c, filter, out, cap, written, n_selected, true);
}

int drp_fanout_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filters, uint32_t nfilters,
                      const drp_change_src *out_rows, uint64_t rows_cap, uint64_t *sel_idx, uint64_t *row_base,
                      const drp_splice *splice) {
  return fanout_device(c, bytes, nbytes, frames, cols, n, filters, nfilters, out_rows, rows_cap, sel_idx, row_base,
                       splice, false);
}

int drp_fanout_staged(drp_ctx *c, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                      uint64_t *out_off, uint64_t *n_selected, uint64_t *blob_row, uint64_t *blob_pos,
                      uint64_t blob_cap, uint64_t *n_blobs) {
  return fanout_staged(c, filters, nfilters, out, cap, out_off, n_selected, blob_row, blob_pos, blob_cap, n_blobs,
                       false);
}

int drp_fanout_latest_device(drp_ctx *c, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                             const drp_changes *cols, uint64_t n, const drp_filter *filters, uint32_t nfilters,
                             const drp_change_src *out_rows, uint64_t rows_cap, uint64_t *sel_idx, uint64_t *row_base) {
  return fanout_device(c, bytes, nbytes, frames, cols, n, filters, nfilters, out_rows, rows_cap, sel_idx, row_base,
                       nullptr, true);
}

int drp_fanout_latest_staged(drp_ctx *c, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                             uint64_t *out_off, uint64_t *n_selected) {
  return fanout_staged(c, filters, nfilters, out, cap, out_off, n_selected, nullptr, nullptr, 0, nullptr, true);
}

}  // extern "C"
