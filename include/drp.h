/*
 * drp.h — C ABI of libdrp, the MI355X (gfx950) batch codec for the
 * dat-replication-protocol hot path: varint-length-prefixed multibuffer
 * framing + protobuf `Change` decode/encode.
 *
 * Reference interface each entry point replaces (mafintosh/dat-replication-protocol v4.1.2):
 *   drp_decode_batch / drp_decode_device
 *       -> Decoder._write/_consume/_onheader/_onchangedata/_onchangeend/_onblobdata
 *          (decode.js:124-133, 144-169, 251-262, 216-249, 205-214, 179-202)
 *          + messages.Change.decode (messages/index.js:5, schema messages/schema.proto:1-8)
 *   drp_carry
 *       -> the decoder's cross-chunk state _header/_ptr/_id/_missing/_buffer/_blob
 *          (decode.js:75-81)
 *   drp_encode_size / drp_encode_batch / drp_encode_device
 *       -> Encoder.change + Encoder._header (encode.js:102-117, 124-137)
 *          + messages.Change.encode (messages/index.js:5)
 *   drp_select_device / drp_relay_staged
 *       -> no reference counterpart (the reference has no relay): a predicate over the decoded
 *          Change columns (schema messages/schema.proto:1-8: subset, change, key) and the encoder
 *          above over the rows it keeps, the received wire serving as the encoder's heap.
 *   drp_fanout_device / drp_fanout_staged
 *       -> no reference counterpart: that select for many filters in one pass (a hub's peers), and
 *          a splice table that keeps the blobs where Encoder.change / Encoder.blob put them between
 *          the Changes (encode.js:77-107).
 *   drp_latest_device / drp_latest_staged
 *       -> no reference counterpart: of the Changes that select keeps, the one with the greatest
 *          `change` per (subset, key) (schema messages/schema.proto:1-8), a hub's fan-in.
 *   drp_fanout_latest_device / drp_fanout_latest_staged
 *       -> no reference counterpart: that latest per key under many filters at once, grouped once
 *          (a hub catching up many peers, each at its own version).
 *   drp_store_init / drp_store_merge_device / drp_store_merge_staged / drp_store_compact /
 *   drp_store_query / drp_store_table_bytes
 *       -> no reference counterpart: the latest Change per (subset, key) over every batch merged so
 *          far, resident in caller-owned device memory in the layout of a decoded batch, so the
 *          relay calls above run over it unchanged (a hub answering "what changed since T?").
 *   drp_store_merge_report_device / drp_store_merge_news_staged / drp_fanout_news_staged
 *       -> no reference counterpart: that merge saying per batch row what became of it, as a type
 *          column under which the batch holds exactly the Changes that changed the store (a relay
 *          forwarding only what was news to it), and the store's rows a stale sender lacks.
 *   drp_store_lookup_device / drp_store_lookup_staged
 *       -> no reference counterpart: a read-only probe of that store by identity, a verdict per
 *          queried key from its `change` against the stored one, the found rows for the encoder (a
 *          multi-get), and a type column under which the store holds exactly the rows the sender of
 *          a have-list lacks (a peer with a plain list of keys and versions catching up).
 *   drp_store_load_device / drp_store_rehash_device
 *       -> no reference counterpart: rows known to be new entered into that store without grouping
 *          or lookup, and its table rebuilt from its rows (a hub growing its store, dropping rows
 *          from it, or restoring it from saved columns after a restart).
 *   drp_order_device
 *       -> no reference counterpart: the rows of every fan-out output in ascending `change` (schema
 *          messages/schema.proto:1-8), cut to a per-peer limit (a catch-up a peer can resume or page).
 *   drp_order_keys_device
 *       -> no reference counterpart: those rows in ascending (key, subset) byte order, cut to a key
 *          range and a page per peer (a listing in key order that a peer can resume after a key).
 *   drp_digest_device / drp_digest_diff_device / drp_select_buckets_device
 *       -> no reference counterpart: a digest of the rows per bucket of identities, the buckets in
 *          which two digests differ, and the select of those buckets' rows (two hubs without a shared
 *          `change` counter reconciling their stores).
 *   drp_digest_refine_device / drp_digest_diff_cells_device / drp_select_refined_device
 *       -> no reference counterpart: a second level of digest cells inside the differing buckets
 *          only, the cells in which two such levels differ, and the select of those cells' rows
 *          (the same reconcile sending a few rows per altered key, not the whole bucket).
 *   drp_stream_stats + drp_index_scan
 *       -> no reference counterpart (the reference is single-stream); they build the
 *          global frame index after the per-GPU stats tables are all-gathered.
 *
 * Rules: every function returns DRP_OK (0) or a negative DRP_E_* code and never
 * throws or aborts across the ABI. All buffers are caller-owned; libdrp never
 * frees caller memory and never returns heap pointers. Pointers passed to the
 * *_device entry points must be device (HBM) pointers; drp_decode_batch /
 * drp_encode_batch accept host or device pointers and stage as needed.
 * One drp_ctx per device; a ctx must not be used from two threads at once.
 */
#ifndef DRP_H
#define DRP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libdrp is built with -fvisibility=hidden: the declarations below are its only exports. */
#pragma GCC visibility push(default)

/* Raised when an existing declaration or layout changes; added symbols do not raise it. */
#define DRP_ABI_VERSION 5

/* ---- return codes -------------------------------------------------------- */
#define DRP_OK 0
#define DRP_E_INVAL (-1)    /* bad argument */
#define DRP_E_HIP (-2)      /* HIP runtime error */
#define DRP_E_NOMEM (-3)    /* device/host allocation failed */
#define DRP_E_CAPACITY (-4) /* output capacity too small */
#define DRP_E_NODEV (-5)    /* no gfx950 device */
#define DRP_E_RETRY (-6)    /* internal: speculation failed and strict re-run also failed */
#define DRP_E_COMM (-7)     /* RCCL error (multi-GPU index) */

/* ---- frame types (the id byte, decode.js:146-161) ------------------------ */
#define DRP_TYPE_CHANGE 1
#define DRP_TYPE_BLOB 2
/* OR-ed into type[] for a blob whose payload continues past the end of the batch */
#define DRP_FRAME_PARTIAL 0x80

/* ---- per-Change flags ---------------------------------------------------- */
#define DRP_F_SUBSET 0x01 /* optional string subset = 1 present */
#define DRP_F_VALUE 0x02  /* optional bytes value = 6 present (value may be empty) */
#define DRP_F_BAD 0x04    /* payload is not a well-formed Change (see err codes) */
#define DRP_F_MISSING 0x08 /* with DRP_F_BAD: a required field (key/change/from/to) is missing */
/* key post-processing (only when drp_changes.key_hash is non-NULL / drp_set_key_post is on): */
#define DRP_F_KEY_ASCII 0x10 /* every key byte < 0x80 */
#define DRP_F_KEY_UTF8 0x20  /* the key bytes are well-formed UTF-8 (so toString('utf-8') is lossless) */

/* ---- stream error codes (first failing frame, see DESIGN.md "policy") ---- */
#define DRP_ERR_NONE 0
#define DRP_ERR_TYPE 1     /* id byte >= 3: 'Protocol error, unknown type: N' (decode.js:159-161) */
#define DRP_ERR_LEN 2      /* length varint 0 on a change/blob frame (reference is chunk-size dependent) */
#define DRP_ERR_VARINT 3   /* header varint longer than 10 bytes or >= 2^64 */
#define DRP_ERR_CHANGE 4   /* malformed Change payload (truncated field, bad wire type, huge varint) */
#define DRP_ERR_REQUIRED 5 /* Change payload lacks a required field (key/change/from/to) */

/* ---- tail kinds: what the caller must carry into the next batch ---------- */
#define DRP_TAIL_NONE 0   /* batch ended on a frame boundary */
#define DRP_TAIL_HEADER 1 /* batch ended inside a frame header: carry bytes [consumed, n) */
#define DRP_TAIL_CHANGE 2 /* batch ended inside a change payload: carry bytes [consumed, n) */
#define DRP_TAIL_BLOB 3   /* batch ended inside a blob payload: blob_remaining bytes still to come */

typedef struct drp_ctx drp_ctx;

/* Frame table, one entry per delivered frame (changes and blobs, in stream order). */
typedef struct drp_frames {
  uint64_t *payload_off; /* offset of payload byte 0 in the batch buffer */
  uint32_t *payload_len; /* declared payload length L-1 (saturates at 0xFFFFFFFF) */
  uint8_t *type;         /* DRP_TYPE_CHANGE / DRP_TYPE_BLOB (| DRP_FRAME_PARTIAL) */
} drp_frames;

/* Change columns, indexed by frame index (the entries of blob frames are unspecified: the device
 * leaves them untouched; a host fetch copies whatever the device columns held there).
 * Offsets are relative to payload_off of the same frame. */
typedef struct drp_changes {
  uint32_t *key_off, *key_len;
  uint32_t *subset_off, *subset_len;
  uint32_t *value_off, *value_len;
  uint64_t *change, *from, *to;
  uint8_t *flags;
  /* optional (NULL = not computed): XXH64 (seed 0) of the key bytes; when set, flags also get
   * DRP_F_KEY_ASCII / DRP_F_KEY_UTF8 (decode.js:210-213 builds a string of every key) */
  uint64_t *key_hash;
} drp_changes;

/* Encoder input: one Change per row; offsets are absolute into `heap`. */
typedef struct drp_change_src {
  const uint64_t *key_off;
  const uint32_t *key_len;
  const uint64_t *subset_off;
  const uint32_t *subset_len;
  const uint64_t *value_off;
  const uint32_t *value_len;
  const uint64_t *change, *from, *to;
  const uint8_t *flags; /* DRP_F_SUBSET / DRP_F_VALUE */
} drp_change_src;

/* Cross-batch carry (mirrors decode.js:75-81). The caller owns the carried bytes:
 * on return, bytes [consumed, n) of the batch must be prepended to the next batch
 * (tail HEADER/CHANGE); for tail BLOB the next batch starts with blob_remaining
 * bytes of blob payload. */
typedef struct drp_carry {
  uint64_t blob_remaining; /* in/out */
  uint64_t consumed;       /* out */
  uint32_t tail_kind;      /* out: DRP_TAIL_* */
  uint32_t reserved;
  uint64_t frame_bytes;    /* out, tail CHANGE: size of the carried frame (header + id + payload), so
                              the caller can collect exactly that many bytes once (decode.js:229-247
                              fills _buffer the same way) instead of re-sending a growing carry */
} drp_carry;

/* Per-stream result of a (multi-)stream decode. */
typedef struct drp_stream_result {
  uint64_t frame_begin;    /* index of the stream's first frame in the output columns */
  uint64_t frames;         /* delivered frames (stop before err_frame) */
  uint64_t changes;        /* delivered change frames */
  uint64_t blobs;          /* delivered blob frames (partial included) */
  uint64_t consumed;       /* stream-relative offset where the carry starts */
  uint64_t blob_remaining; /* tail BLOB: payload bytes still to come */
  uint64_t err_frame;      /* UINT64_MAX if no error, else stream-relative index of failing frame */
  uint32_t err_code;       /* DRP_ERR_* */
  uint32_t err_detail;     /* DRP_ERR_TYPE: the id byte */
  uint32_t tail_kind;      /* DRP_TAIL_* */
  uint32_t reserved;
  uint64_t tail_frame_bytes; /* tail CHANGE: header + id + payload bytes of the carried frame */
} drp_stream_result;

/* The 32-byte per-stream record exchanged by the multi-GPU all-gather. */
typedef struct drp_stream_stats {
  uint64_t frames, changes, blobs, wire_bytes;
} drp_stream_stats;

/* Timing of the last device launch sequence on a ctx (HIP events, milliseconds). */
typedef struct drp_timing {
  float decode_ms;   /* main decode kernel */
  float finalize_ms; /* per-stream finalize kernel */
  float total_ms;    /* memset + decode + finalize (+ strict re-run if any) */
  uint32_t strict_reruns; /* 1: the speculative decode fell back to the exact kernel */
  uint32_t spec_repairs;  /* verify passes that repaired failed predictions in place */
  uint32_t exact_retries; /* 1: the exact kernel's bounded look-back wait expired and it was re-run */
  uint32_t verify_relisted; /* tiles verify_lite handed to verify_counts (a re-walk or a longer look-back) */
  uint32_t seg_repairs;     /* streams whose claims the segmented repair recomputed (miss cascades) */
  uint32_t reserved;
  /* host-batch calls (drp_decode_stage / drp_decode_fetch / drp_decode_batch), wall clock: */
  float h2d_ms;   /* staging the batch into HBM */
  float d2h_ms;   /* copying the columns back (drp_decode_fetch; a pipelined batch: the rows left after its copy) */
  uint64_t h2d_bytes;   /* bytes of the last host batch staged into HBM */
  uint64_t h2d_skipped; /* its blob payload bytes never staged (pass-through, drp_set_blob_skip) */
  uint64_t host_copied; /* bytes of a chunked batch gathered on the host (drp_decode_stage_v) */
} drp_timing;

/* ---- context ------------------------------------------------------------- */
int drp_abi_version(void);
/* Number of HIP devices visible to the process (0 when none; gfx950 is checked by drp_open). */
int drp_device_count(int *n);
int drp_open(int device, drp_ctx **out);
void drp_close(drp_ctx *ctx);
/* The hipStream_t (as void*) all kernels of this ctx are launched on. */
void *drp_stream(drp_ctx *ctx);
/* The HIP device of this ctx. */
int drp_device(drp_ctx *ctx);
int drp_synchronize(drp_ctx *ctx);
int drp_last_timing(drp_ctx *ctx, drp_timing *out);
/* Tunables (0 = default 8192). tile_bytes is 4096 or 8192 (64 lanes x 64 or 128 bytes). */
int drp_set_tile(drp_ctx *ctx, uint32_t tile_bytes);
/* 1: always run the exact decode kernel (per-tile transfer functions); 0 (default): run the
 * speculate-and-verify kernel and fall back to the exact one when a prediction fails.
 * Results are identical either way; drp_timing.strict_reruns reports a fallback. */
int drp_set_exact(drp_ctx *ctx, int exact);
/* Key post-processing on every decode of the ctx (drp_keys.hip):
 * DRP_KEY_POST_HASH (1): the key hash column (drp_decode_stage: fetched when the caller's
 *   drp_changes.key_hash is non-NULL) and the key flags DRP_F_KEY_ASCII / DRP_F_KEY_UTF8;
 * DRP_KEY_POST_FLAGS (2): the key flags only (no hash column);
 * DRP_KEY_POST_OFF (0, default): neither. */
#define DRP_KEY_POST_OFF 0
#define DRP_KEY_POST_HASH 1
#define DRP_KEY_POST_FLAGS 2
int drp_set_key_post(drp_ctx *ctx, int mode);
/* Look-back composes exact inclusive exits only, never the per-tile maps agg_t. Test hook. */
int drp_set_strict(drp_ctx *ctx, int strict);
/* Host batches (drp_decode_stage / drp_decode_batch): blob payloads are pass-through ranges into
 * the caller's buffer, so their bytes need not reach HBM (decode.js:179-202 only slices them).
 * DRP_BLOB_SKIP_AUTO (default): a ctx whose last batch was mostly blob payload stages the next
 * batches in pieces, each ending a little past the next blob header (sized from the runs between
 * blobs seen so far); a piece that ends inside a blob resumes after it, skipping its payload.
 * DRP_BLOB_SKIP_ALWAYS: every host batch in pieces; DRP_BLOB_SKIP_OFF: every batch staged whole.
 * Results are identical in every mode; drp_timing.h2d_bytes / h2d_skipped report the bytes. */
#define DRP_BLOB_SKIP_OFF 0
#define DRP_BLOB_SKIP_AUTO 1
#define DRP_BLOB_SKIP_ALWAYS 2
int drp_set_blob_skip(drp_ctx *ctx, int mode);
/* Device scratch bytes needed to decode `n` bytes split into `nstreams` streams. */
uint64_t drp_decode_scratch_bytes(drp_ctx *ctx, uint64_t n, uint64_t nstreams);

/* Page-locked host memory (hipHostMalloc) for staging host batches: a batch the caller assembles
 * there is copied into HBM by DMA at the full PCIe rate instead of through the runtime's pageable
 * bounce buffer (the N-API addon coalesces small writes into such blocks). */
int drp_host_alloc(uint64_t bytes, void **out);
void drp_host_free(void *p);

/* ---- decode -------------------------------------------------------------- */
/* Decode `nstreams` independent streams laid end to end in `bytes` (device ptr, 16-byte
 * aligned, `nbytes` long).
 * stream_off[nstreams+1] (device) gives stream s = bytes[stream_off[s], stream_off[s+1]);
 * entry[nstreams] (device, may be NULL = all zero) is the stream-relative offset of the
 * first frame header (skips a blob continuation). Frames of all streams are written to
 * `frames`/`cols` (device) in stream order; per-stream results go to results[] (device).
 * Runs on drp_stream(ctx) and returns after completion (the speculation check needs the
 * result); capacity `cap` frames (DRP_E_CAPACITY if more were found). */
int drp_decode_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes,
                      const uint64_t *stream_off, const uint64_t *entry, uint64_t nstreams,
                      const drp_frames *frames, const drp_changes *cols, uint64_t cap,
                      drp_stream_result *results);

/* Synchronous single-stream decode of one batch (host or device pointers).
 * carry->blob_remaining in: leading blob continuation; out: carry for the next batch.
 * Returns frames delivered in *n_frames, first failing frame in *err_frame
 * (UINT64_MAX if none) with *err_code and *err_detail. A leading blob continuation is
 * reported as frame 0 with type DRP_TYPE_BLOB|0x40 (continuation).
 * A host batch of 256 MiB or more in page-locked memory is decoded as it is copied (128 MiB DMA
 * chunks on a second stream of the ctx, one piece decoded per chunk; the rows of each piece are
 * copied into the host columns by a ctx-internal worker thread during the next chunk's copy):
 * the results are those of one whole-batch decode, and the call still returns only when every
 * row is in the columns. A ctx stays single-threaded for its callers. */
#define DRP_FRAME_CONT 0x40
int drp_decode_batch(drp_ctx *ctx, const uint8_t *bytes, uint64_t n, drp_carry *carry,
                     const drp_frames *frames, const drp_changes *cols, uint64_t cap,
                     uint64_t *n_frames, uint64_t *err_frame, uint32_t *err_code,
                     uint32_t *err_detail);

/* Two-step form of drp_decode_batch for callers that size their host columns from the
 * result (the N-API addon, which runs it on a worker thread): drp_decode_stage decodes one
 * host batch into device columns owned by the ctx (capacity grows as needed) and reports the
 * same counts, error and carry as drp_decode_batch; drp_decode_fetch then copies rows
 * [first, first + rows) into caller-owned HOST columns. Rows = *n_frames, plus one for a
 * malformed Change (DRP_ERR_CHANGE / DRP_ERR_REQUIRED: its flags say why). The staged result
 * stays valid until the next decode call on the ctx. A leading blob continuation's bytes
 * (carry->blob_remaining) are never copied to the device. */
int drp_decode_stage(drp_ctx *ctx, const uint8_t *bytes, uint64_t n, drp_carry *carry,
                     uint64_t *n_frames, uint64_t *err_frame, uint32_t *err_code, uint32_t *err_detail);
int drp_decode_fetch(drp_ctx *ctx, const drp_frames *frames, const drp_changes *cols, uint64_t first,
                     uint64_t rows);
/* drp_decode_fetch into one caller-owned HOST block [block, block + block_bytes) that libdrp may
 * write anywhere in (padding between the columns included): column k at block + col_off[k], in
 * the order payload_off, payload_len, type, key_off, key_len, subset_off, subset_len, value_off,
 * value_len, change, from, to, flags, key_hash (col_off[13] = UINT64_MAX: no key hash column).
 * The columns are packed on the device in that layout and copied in one transfer (page-locked
 * blocks: one DMA instead of one per column). Replaces the same per-frame loop as
 * drp_decode_fetch (decode.js:144-169 with messages.Change.decode). */
#define DRP_FETCH_COLS 14
int drp_decode_fetch_block(drp_ctx *ctx, void *block, uint64_t block_bytes, const uint64_t *col_off, uint64_t first,
                           uint64_t rows);
/* drp_decode_fetch_block with column forms for a JavaScript host: flags DRP_FETCH_F64 writes
 * payload_off, change, from and to as IEEE doubles (the Numbers decode.js hands out: exact below
 * 2^53, the nearest double above, as a host (double) cast rounds), converted on the device before
 * the transfer. flags 0: drp_decode_fetch_block. */
#define DRP_FETCH_F64 1u
int drp_decode_fetch_block_ex(drp_ctx *ctx, void *block, uint64_t block_bytes, const uint64_t *col_off,
                              uint64_t first, uint64_t rows, uint32_t flags);
/* The keys of the staged rows [first, first + rows) whose key the key post-processing flagged
 * ASCII (drp_set_key_post; Change rows without DRP_F_BAD), end to end: kp[r] = the text length
 * before row r (every row), text = those keys (at most text_cap bytes), *text_len = its length.
 * Built on the device from the staged batch (a JavaScript host makes one string of it and cuts
 * each key as a substring, the same string the key bytes' UTF-8 decode would give). text = NULL:
 * only kp and *text_len. DRP_E_CAPACITY: the text is longer than text_cap (kp and *text_len are
 * still written). DRP_E_INVAL when the batch was staged in more than one piece (blob skipping:
 * its earlier pieces are no longer on the device) or the keys were not flagged. Replaces the key
 * string of messages.Change.decode (decode.js:205-214). */
int drp_decode_fetch_keys(drp_ctx *ctx, uint64_t first, uint64_t rows, uint32_t *kp, char *text, uint64_t text_cap,
                          uint64_t *text_len);
/* drp_decode_stage over a batch the caller holds as chunks (its queued writes), laid end to end:
 * the caller never concatenates them. The ranges the decode stages into HBM (all of the batch,
 * or with blob skipping everything but the blob payloads) are gathered from the chunks into
 * page-locked memory of the ctx and copied by DMA; drp_timing.host_copied reports the bytes
 * gathered, so blob payloads are copied neither on the host nor to the device. Offsets in the
 * result are batch offsets (the chunks' concatenation). Replaces the per-write _consume loop's
 * input side (decode.js:144-169: each written chunk is parsed in place). */
typedef struct drp_chunk {
  const uint8_t *bytes;
  uint64_t n;
} drp_chunk;
int drp_decode_stage_v(drp_ctx *ctx, const drp_chunk *chunks, uint64_t nchunks, drp_carry *carry,
                       uint64_t *n_frames, uint64_t *err_frame, uint32_t *err_code, uint32_t *err_detail);

/* ---- encode -------------------------------------------------------------- */
/* Wire size of encoding rows [0,n) as change frames (varint(len+1) 0x01 payload). */
int drp_encode_size(drp_ctx *ctx, const drp_change_src *src, uint64_t n, uint64_t *wire_bytes);
/* Device pointers; asynchronous. frame_off[n+1] (device scratch, written) receives the
 * exclusive prefix of frame sizes (frame_off[n] = wire bytes). A row whose key/subset/value
 * range leaves [0, heap_bytes) sets frame_off[n] = UINT64_MAX and nothing is written. */
int drp_encode_device(drp_ctx *ctx, const drp_change_src *src, const uint8_t *heap, uint64_t heap_bytes,
                      uint64_t n, uint64_t *frame_off, uint8_t *out, uint64_t cap);
/* Synchronous; host or device pointers. DRP_E_INVAL if a row's range leaves the heap. Host columns
 * or a host heap are staged through the ctx's input staging, which ends a staged decode's validity
 * for drp_relay_staged / drp_decode_fetch_keys (see drp_relay_staged); drp_encode_size likewise. */
int drp_encode_batch(drp_ctx *ctx, const drp_change_src *src, const uint8_t *heap,
                     uint64_t heap_bytes, uint64_t n, uint8_t *out, uint64_t cap,
                     uint64_t *written);

/* ---- select + re-encode (relay) ------------------------------------------- */
/* Which decoded Changes a relay keeps. A row is selected iff it is a Change frame
 * ((type & 0x3F) == DRP_TYPE_CHANGE), DRP_F_BAD is clear and every condition enabled in `flags`
 * holds (the conditions AND together). flags == 0 (or a NULL filter) selects every well-formed
 * Change: the canonicalising re-encode. Unknown flag bits, DRP_SEL_SUBSET_EQ together with
 * DRP_SEL_SUBSET_NONE, and a byte string longer than DRP_SEL_MAX_BYTES are DRP_E_INVAL. */
#define DRP_SEL_CHANGE_RANGE 0x01 /* change_min <= change <= change_max (unsigned; min > max: nothing) */
#define DRP_SEL_SUBSET_EQ 0x02    /* subset present and its bytes equal subset[0, subset_len) (an empty
                                     subset matches subset_len == 0; an absent one never matches) */
#define DRP_SEL_SUBSET_NONE 0x04  /* subset absent */
#define DRP_SEL_KEY_PREFIX 0x08   /* key_len >= key_prefix_len and the key starts with key_prefix (length 0:
                                     every key) */
#define DRP_SEL_MAX_BYTES 256
typedef struct drp_filter {
  uint32_t flags; /* DRP_SEL_* */
  uint32_t subset_len;
  uint32_t key_prefix_len;
  uint32_t reserved;
  uint64_t change_min, change_max;
  const uint8_t *subset;     /* HOST pointers (read before the call returns); may be NULL when the */
  const uint8_t *key_prefix; /* length is 0 */
} drp_filter;

/* The selected rows of decoded rows [0, n), in stream order (a stable compaction), as encoder rows:
 * out_rows' offsets are absolute into `bytes` (payload_off + key_off, likewise subset and value),
 * flags are masked to DRP_F_SUBSET | DRP_F_VALUE (the key post-processing bits never reach the
 * encoder), so drp_encode_device(ctx, out_rows, bytes, nbytes, *n_selected, ...) re-encodes them
 * with the wire as its heap and no payload byte copied in between. Device pointers only;
 * asynchronous on drp_stream(ctx). The arrays behind out_rows are caller-owned WRITABLE device
 * memory of n entries each: they are written through the const pointers of drp_change_src (rows
 * [0, *n_selected); the rest is left untouched). sel_idx (device, n entries, may be NULL) receives
 * the source row of each selected row, n_selected (device) their count. frames / cols may be the
 * flat multi-stream output of drp_decode_device with n = the rows it wrote (the streams' delivered
 * frames end to end). A row whose key / subset range leaves [0, nbytes) is never read and never
 * matches a byte condition. */
int drp_select_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filter, const drp_change_src *out_rows,
                      uint64_t *sel_idx, uint64_t *n_selected);
/* Select over the delivered rows of the batch last staged by drp_decode_stage / drp_decode_stage_v
 * (nothing at or after an error frame, nor a malformed Change) and encode the selection as change
 * frames into `out` (host or device pointer, capacity cap) with the staged wire as the heap.
 * Synchronous. *written = the size needed, also when DRP_E_CAPACITY is returned (nothing is
 * written to out then); *n_selected = the rows kept. The staged result stays valid: the caller can
 * still drp_decode_fetch the frame table to forward blobs and to carry the tail. The same bytes in
 * every drp_set_blob_skip mode. DRP_E_INVAL when no staged batch is held: before any stage, after
 * a stage that failed, and once the staged bytes have left the device. They share the ctx's input
 * staging with the encoder, so a drp_encode_batch or drp_encode_size whose columns or heap are HOST
 * memory ends the staged batch for drp_relay_staged and drp_decode_fetch_keys (both then return
 * DRP_E_INVAL; drp_decode_fetch* still work, the columns are kept elsewhere), as does the next
 * decode call. drp_encode_device, drp_select_device and an encode from device memory do not. */
int drp_relay_staged(drp_ctx *ctx, const drp_filter *filter, uint8_t *out, uint64_t cap, uint64_t *written,
                     uint64_t *n_selected);

/* ---- fan-out: many filters over one decoded batch ------------------------- */
/* A hub relays one received batch to many peers, each with its own filter. The two entry points
 * below evaluate up to DRP_FANOUT_MAX filters in one pass over the decoded rows (every column is
 * read once, whatever the number of filters) and lay the kept rows of the filters end to end, so
 * one encode produces every peer's bytes. No reference counterpart (the reference has no relay);
 * the splice table restores the order encode.js:77-100 keeps between Changes and blobs. */
#define DRP_FANOUT_MAX 64

/* Optional splice outputs of drp_fanout_device (device pointers): where the blob frames of rows
 * [0, n) (every row with (type & 0x3F) == DRP_TYPE_BLOB, partial ones included) belong in each
 * output. */
typedef struct drp_splice {
  uint64_t *blob_row;  /* blob_cap entries: source row of each blob frame, in stream order */
  uint64_t *blob_rank; /* nfilters * blob_cap: [f * blob_cap + j] = rows of output f before blob j */
  uint64_t *n_blobs;   /* one entry: the true count (nothing is written to the arrays if > blob_cap) */
  uint64_t blob_cap;
} drp_splice;

/* drp_select_device for nfilters filters at once (1 .. DRP_FANOUT_MAX; filters[f].flags == 0 selects
 * every well-formed Change). Output f is rows [row_base[f], row_base[f + 1]) of out_rows and of
 * sel_idx (device, may be NULL), each a stable compaction as drp_select_device's; row_base (device,
 * nfilters + 1 entries) is always written and carries the true counts. out_rows' arrays and sel_idx
 * hold rows_cap entries: if row_base[nfilters] > rows_cap nothing is written to them, otherwise rows
 * at or beyond row_base[nfilters] are left untouched. drp_encode_device(ctx, out_rows, bytes, nbytes,
 * row_base[nfilters], frame_off, ...) then encodes every output in one call: output f is
 * out[frame_off[row_base[f]], frame_off[row_base[f + 1]]). splice may be NULL. Device pointers only
 * (filters and the drp_splice struct itself are HOST memory, read before the call returns);
 * asynchronous on drp_stream(ctx). DRP_E_INVAL: nfilters out of range, a filter drp_select_device
 * rejects, the NULL pointers drp_select_device rejects, a NULL row_base. */
int drp_fanout_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filters, uint32_t nfilters,
                      const drp_change_src *out_rows, uint64_t rows_cap, uint64_t *sel_idx, uint64_t *row_base,
                      const drp_splice *splice);
/* drp_relay_staged for nfilters filters at once, over the batch last staged (the same rows, the same
 * validity rules and DRP_E_INVAL cases, the same bytes in every drp_set_blob_skip mode). Synchronous.
 * The outputs lie end to end in `out` (host or device pointer, capacity cap): output f is
 * out[out_off[f], out_off[f + 1]) and holds n_selected[f] Changes (out_off: HOST, nfilters + 1;
 * n_selected: HOST, nfilters). DRP_E_CAPACITY: nothing is written to out, out_off[nfilters] = the
 * size needed, n_selected is valid. Splice table (blob_row NULL: none; all HOST): blob_row[j] = the
 * row, as drp_decode_fetch numbers them, of the batch's j-th blob frame (a leading continuation,
 * fetch row 0 with DRP_FRAME_CONT, is not listed: it precedes every output); blob_pos[f * blob_cap +
 * j] = the byte offset within output f at which that frame belongs. *n_blobs = the true count; if it
 * exceeds blob_cap the two arrays are not written and the call still succeeds for out. */
int drp_fanout_staged(drp_ctx *ctx, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                      uint64_t *out_off, uint64_t *n_selected, uint64_t *blob_row, uint64_t *blob_pos,
                      uint64_t blob_cap, uint64_t *n_blobs);

/* ---- latest per key: one Change per (subset, key) (relay fan-in) ----------- */
/* A replication feed is a log: the same (subset, key) is written again and again, and a hub that
 * catches a peer up, or merges the feeds of several peers, wants every key's current Change only.
 * No reference counterpart (the reference has no relay); the fields read are subset, key and change
 * of messages/schema.proto:1-8.
 *   Candidates: the rows drp_select_device selects with the same filter (a NULL filter or flags == 0:
 * every well-formed Change) whose key range and, with DRP_F_SUBSET, subset range lie inside
 * [0, nbytes); a row whose range leaves the wire is never read and is no candidate.
 *   Identity: subset presence (DRP_F_SUBSET), the subset bytes and the key bytes, as whole byte
 * strings: an absent and a present empty subset differ, "a" and "ab" differ, an empty key is a key.
 *   Winner: of the candidates of one identity the one with the greatest `change` (unsigned 64-bit);
 * on a tie the greatest row index (the later row of a stream, the later stream of flat multi-stream
 * columns). With DRP_SEL_CHANGE_RANGE and change_max = T the result is the snapshot at version T. */

/* drp_select_device with that reduction behind the predicate: the winners of rows [0, n) in
 * increasing row order, written as drp_select_device writes its rows (out_rows' offsets absolute
 * into `bytes`, flags masked to DRP_F_SUBSET | DRP_F_VALUE, sel_idx and n_selected as there). The
 * result is a function of the input alone. Device pointers only; asynchronous on drp_stream(ctx).
 * The argument rules and DRP_E_INVAL cases are drp_select_device's. The grouping table comes from
 * the ctx's scratch (8 bytes per row and 24 bytes for each of the 2 n slots, rounded up to a power
 * of two): DRP_E_NOMEM if it cannot be allocated. */
int drp_latest_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filter, const drp_change_src *out_rows,
                      uint64_t *sel_idx, uint64_t *n_selected);
/* drp_relay_staged with the latest-per-key step between select and encode: over the same rows of
 * the batch last staged, with the same validity rules and DRP_E_INVAL cases, the same
 * DRP_E_CAPACITY contract (*written = the size needed, nothing written to out) and the same bytes
 * in every drp_set_blob_skip mode. Synchronous. *n_selected = the winners. */
int drp_latest_staged(drp_ctx *ctx, const drp_filter *filter, uint8_t *out, uint64_t cap, uint64_t *written,
                      uint64_t *n_selected);
/* The row hash of the two calls above is ANDed with `mask` before it picks a slot of the grouping
 * table (default: all ones; 0: every row starts at the same slot). Results are identical for
 * every mask. Test hook. */
int drp_set_latest_hash_mask(drp_ctx *ctx, uint64_t mask);

/* ---- fan-out of latest per key: many snapshots over one grouping ----------- */
/* A hub that catches up many peers at once wants, for peer f, the snapshot under that peer's filter
 * (its version T_f as DRP_SEL_CHANGE_RANGE, its subset, its key prefix). Output f of the two calls
 * below is exactly what drp_latest_device returns for filters[f] over the same rows: the same
 * candidates, identity, winner, row order, wire-bounds rule and flag masking. The part that does not
 * depend on the filter is done once: the predicates in one pass over the columns (as drp_fanout_device),
 * and the grouping (the hash of every key, the table probes, the byte compares) over the rows that
 * at least one filter keeps; only the reduction to the greatest (change, row) runs per filter.
 * No reference counterpart (the reference has no relay); the fields read are subset, key and change
 * of messages/schema.proto:1-8. */

/* drp_fanout_device without the splice argument (a snapshot has no blobs to place) and with that
 * reduction behind every predicate: output f is rows [row_base[f], row_base[f + 1]) of out_rows and of
 * sel_idx (device, may be NULL), the winners under filters[f] in increasing row order; row_base
 * (device, nfilters + 1 entries) is always written and carries the true counts. If
 * row_base[nfilters] > rows_cap nothing is written to out_rows or sel_idx, otherwise entries at or
 * beyond row_base[nfilters] are left untouched; one drp_encode_device over row_base[nfilters] rows
 * encodes every output. The result is a function of the input alone. Device pointers only (filters
 * is HOST memory, read before the call returns); asynchronous on drp_stream(ctx), no host
 * synchronisation inside. The DRP_E_INVAL cases are drp_fanout_device's. Scratch, from the ctx's
 * (DRP_E_NOMEM if it cannot be allocated): drp_fanout_device's, 8 bytes per row, 8 bytes for each of
 * the 2 n slots, rounded up to a power of two, 2 bits per row, and per row 16 bytes per filter of one
 * reduction pass (min(nfilters, 8) by default: 128 bytes per row at most). */
int drp_fanout_latest_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                             const drp_changes *cols, uint64_t n, const drp_filter *filters, uint32_t nfilters,
                             const drp_change_src *out_rows, uint64_t rows_cap, uint64_t *sel_idx, uint64_t *row_base);
/* drp_fanout_staged without the four blob arguments and with that reduction: over the same delivered
 * rows of the batch last staged, with the same validity rules and DRP_E_INVAL cases and the same
 * bytes in every drp_set_blob_skip mode; output f equals drp_latest_staged's bytes for filters[f].
 * Synchronous. out: host or device pointer; out_off (HOST, nfilters + 1) and n_selected (HOST,
 * nfilters) as there. DRP_E_CAPACITY: nothing is written to out, out_off[nfilters] = the size needed,
 * n_selected is valid. The staged batch stays valid. */
int drp_fanout_latest_staged(drp_ctx *ctx, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                             uint64_t *out_off, uint64_t *n_selected);
/* Filters one reduction pass of the two calls above handles (0: the default; above nfilters: all in
 * one pass). Results are identical for every value; the scratch grows with it. Test hook, as
 * drp_set_latest_hash_mask, which applies to the two calls as well. */
int drp_set_fanout_latest_pass(drp_ctx *ctx, uint32_t filters_per_pass);

/* ---- store: the latest Change per key, resident on the device -------------- */
/* The calls above reduce one decoded batch. A hub receives batches for as long as it runs, and a
 * peer asks it "what has changed since my version T?". The store is the current state the batches
 * merge into: one row per identity (subset presence, subset bytes, key bytes), holding the winner of
 * drp_latest_device over everything merged so far. No reference counterpart (the reference has no
 * relay); the fields read are those of messages/schema.proto:1-8.
 *   The store lives in caller-owned device memory; libdrp allocates nothing for it and there is no
 * open or close. Its rows have the layout of a decoded batch, with the arena in the wire's place:
 * (s->arena, s->arena_bytes, &s->frames, &s->cols) is a valid input of drp_select_device,
 * drp_fanout_device, drp_latest_device, drp_fanout_latest_device and (through their rows)
 * drp_encode_device. frames.type is 0 at and beyond info.rows, so a caller may pass n = max_keys
 * to any of them without reading the count back: the unused rows are no Changes and select nothing.
 * A catch-up of K peers at versions T_f is one drp_fanout_device with DRP_SEL_CHANGE_RANGE =
 * [T_f + 1, 2^64 - 1] over that view and one drp_encode_device.
 *   Stored form of row r: the payload key | subset | value at arena[payload_off[r]] (a multiple of
 * 16), payload_len = key_len + subset_len + value_len, type = DRP_TYPE_CHANGE, key_off = 0,
 * subset_off = key_len, value_off = key_len + subset_len (an absent field has length 0), change /
 * from / to copied, flags = the source's & (DRP_F_SUBSET | DRP_F_VALUE). An allocation is
 * payload_len rounded up to 16 bytes; bytes past the payload are zero. Rows stand in the order in
 * which their identities first entered and keep their index for good. */
typedef struct drp_store_info { /* one record in device memory, written by the calls below */
  uint64_t rows;       /* identities held = rows of frames / cols in use */
  uint64_t arena_used; /* bytes of the arena handed out so far */
  uint64_t arena_dead; /* of those, bytes of payloads since replaced */
  uint64_t merges;     /* merges applied (a refused one is not counted) */
  /* the last merge / compact: */
  uint64_t winners, inserted, replaced, unchanged, stale, skipped;
  uint64_t refused; /* 1: it did not fit; nothing but the fields of this group changed */
  uint64_t need_rows, need_bytes; /* rows it would have added, arena bytes it would have taken */
  uint64_t reserved; /* 0 (the record is 112 bytes) */
} drp_store_info;

typedef struct drp_store { /* HOST struct of DEVICE pointers, read before a call returns */
  uint8_t *arena; /* 16-byte aligned */
  uint64_t arena_bytes;
  drp_frames frames; /* max_keys entries each */
  drp_changes cols;  /* max_keys entries each; cols.key_hash is ignored */
  uint64_t max_keys; /* 1 .. 2^31 */
  uint64_t *table;   /* drp_store_table_bytes(max_keys) bytes */
  drp_store_info *info;
  uint64_t reserved; /* not read (the struct is 160 bytes) */
} drp_store;

/* 8 bytes for each slot of the identity table: a power of two >= 2 * max_keys, at least 2.
 * 0 if max_keys is 0 or above 2^31. */
uint64_t drp_store_table_bytes(uint64_t max_keys);
/* An empty store: the table, the info record and frames.type[0, max_keys) zeroed. Asynchronous on
 * drp_stream(ctx). DRP_E_INVAL: a NULL pointer in *s, an arena that is not 16-byte aligned,
 * max_keys out of range. */
int drp_store_init(drp_ctx *ctx, const drp_store *s);
/* Merge the decoded rows [0, n) of a batch (bytes, frames, cols: drp_latest_device's arguments and
 * DRP_E_INVAL cases) into the store.
 *   Winners: exactly the rows drp_latest_device returns for (bytes, nbytes, frames, cols, n, filter).
 * A winner with DRP_F_VALUE whose value range leaves [0, nbytes) is never read: it counts as
 * `skipped` and the store keeps what it had (so does one whose three lengths sum past 2^32 - 16).
 *   Every other winner is looked up by identity. Absent: `inserted` as row info.rows + its rank among
 * the inserted winners in batch-row order. Present with a greater stored change: `stale`. Present
 * with equal change, from, to, flags & (SUBSET | VALUE) and value bytes: `unchanged`, nothing is
 * written (a batch delivered twice costs no arena). Otherwise `replaced` (a greater change, or an
 * equal one with different content: the later arrival wins, as the later row wins in
 * drp_latest_device): the row keeps its index, its columns are rewritten, a fresh payload is
 * appended to the arena and the old allocation is added to arena_dead.
 *   All or nothing: if rows + inserted > max_keys or arena_used + need_bytes > arena_bytes the merge
 * is refused: refused = 1, need_rows and need_bytes are set with the other fields of the record's
 * last-merge group, and nothing else changes (the table neither). The verdict is taken on the
 * device: the call has no host synchronisation and returns DRP_OK either way; read the record with
 * drp_store_query. After merges B1 .. Bk under one filter, none refused or skipped, the rows hold
 * exactly the winners of drp_latest_device over B1 | ... | Bk under that filter.
 *   Device pointers only; asynchronous on drp_stream(ctx). Scratch from the ctx's (DRP_E_NOMEM if it
 * cannot be had): drp_latest_device's, and per row of the batch 80 bytes of winner rows and 32
 * bytes of merge state. */
int drp_store_merge_device(drp_ctx *ctx, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                           const drp_frames *frames, const drp_changes *cols, uint64_t n, const drp_filter *filter);
/* That merge over the delivered rows of the batch last staged (the rows, validity rules and
 * DRP_E_INVAL cases of drp_latest_staged; the same store in every drp_set_blob_skip mode).
 * Synchronous: *info_host (HOST, may be NULL) receives the record; DRP_E_CAPACITY if the merge was
 * refused (*info_host is still filled). The staged batch stays valid. */
int drp_store_merge_staged(drp_ctx *ctx, const drp_store *s, const drp_filter *filter, drp_store_info *info_host);
/* Copy the live payloads into arena2 (device, 16-byte aligned, arena2_bytes long, not overlapping
 * the arena) in row order, rewrite payload_off, and set arena_used to the live total and arena_dead
 * to 0. The table maps identities to rows and is not touched. If the live total exceeds
 * arena2_bytes the compact is refused on the device (refused = 1, need_bytes = the live total,
 * nothing else changed); otherwise refused = 0 and the caller puts arena2 and arena2_bytes into its
 * drp_store. The other fields of the last-merge group are zeroed; merges is not counted.
 * Asynchronous on drp_stream(ctx), returns DRP_OK either way. */
int drp_store_compact(drp_ctx *ctx, const drp_store *s, uint8_t *arena2, uint64_t arena2_bytes);
/* Wait for the ctx's stream and copy the record to *info_host (HOST). */
int drp_store_query(drp_ctx *ctx, const drp_store *s, drp_store_info *info_host);
/* drp_set_latest_hash_mask applies to the store's table as well (test hook): a store must see one
 * mask from drp_store_init on, for its whole life. */

/* ---- merge report: per-row outcomes, the news view and the stale reply -------------------- */
/* A merge counts its outcomes in the record; a hub that passes a batch on needs to know which rows
 * they were. "Forward only what was news to me" is the rule of any relay or gossip topology: relaying
 * the whole batch sends round again what two upstream peers, or an echo, deliver twice. And a `stale`
 * winner says the sender lacks a row the hub holds. The report exposes both in a form every relay call
 * above takes unchanged. No reference counterpart (the reference has no relay); the fields read are
 * those of messages/schema.proto:1-8.
 *   The merge itself is exactly drp_store_merge_device's: the same winners, outcomes and all-or-nothing
 * verdict, the same store bytes and info record; a NULL report, or one whose outputs are all NULL, is
 * that call. Asynchronous on drp_stream(ctx), no host synchronisation inside.
 *   outcome[r], for every batch row r in [0, n): DRP_MERGE_NONE if r is not one of the winners
 * drp_latest_device returns for these arguments, otherwise that winner's outcome as the store section
 * defines it. After a refused merge the classification is still written (INSERTED and REPLACED then
 * mean "would have been"); the caller reads `refused` from the record.
 *   news_type[r], a replacement for frames->type: DRP_TYPE_CHANGE where the merge was not refused and
 * outcome[r] is INSERTED or REPLACED; with DRP_REPORT_KEEP_BLOBS a row with (type[r] & 0x3F) ==
 * DRP_TYPE_BLOB keeps type[r] as it is (DRP_FRAME_PARTIAL with it; after a refusal too); 0 everywhere
 * else. So (bytes, nbytes, {payload_off, payload_len, news_type}, cols, n) is a decoded batch holding
 * exactly the Changes that changed the store: drp_select_device, drp_fanout_device with its splice
 * table, drp_latest_device, drp_order_device behind them and drp_digest_device run over it unchanged,
 * and not one of the other twelve columns is copied. The news rows number inserted + replaced of the
 * record. news_type == frames->type (aliasing) is DRP_E_INVAL.
 *   Reply: the stale winners in batch-row order; for each the store's row of that identity (the one
 * whose greater `change` beat it), written as drp_select_device writes that row over the store's view:
 * offsets absolute into s->arena (payload_off, + key_len, + key_len + subset_len), flags masked to
 * DRP_F_SUBSET | DRP_F_VALUE; reply_idx[j] is the store row. *n_reply always carries the true count;
 * if it exceeds reply_cap nothing is written to the arrays (drp_fanout_device's rows_cap convention),
 * otherwise entries at or beyond it are left untouched. drp_encode_device(ctx, reply_rows, s->arena,
 * s->arena_bytes, *n_reply, ...) gives the bytes to send back to that peer. The reply is written
 * after a refused merge too (a stale row is stale either way); its offsets hold until the next
 * drp_store_compact.
 *   Entries of outcome and news_type at or beyond n are left untouched.
 *   DRP_E_INVAL: drp_store_merge_device's cases; unknown flag bits; reply_rows without n_reply; with
 * reply_cap > 0 a NULL array in reply_rows; the aliasing above. Scratch, on top of the merge's and
 * only when asked for: 8 bytes per batch row (the winners' source rows) for outcome or news_type, 8
 * bytes per 256 rows (the stale scan) for the reply. */
#define DRP_MERGE_NONE 0 /* the row is no winner: no candidate, or beaten inside the batch */
#define DRP_MERGE_INSERTED 1
#define DRP_MERGE_REPLACED 2
#define DRP_MERGE_UNCHANGED 3
#define DRP_MERGE_STALE 4
#define DRP_MERGE_SKIPPED 5
#define DRP_REPORT_KEEP_BLOBS 0x01

typedef struct drp_merge_report { /* HOST struct of DEVICE pointers, read before the call returns; 64 bytes */
  uint32_t flags, reserved;
  uint8_t *outcome;                 /* n entries, may be NULL */
  uint8_t *news_type;               /* n entries, may be NULL */
  const drp_change_src *reply_rows; /* HOST pointer to a struct of writable device arrays, reply_cap entries each; NULL: no reply */
  uint64_t *reply_idx;              /* reply_cap entries, may be NULL */
  uint64_t *n_reply;                /* one entry; required with reply_rows */
  uint64_t reply_cap;
  uint64_t reserved2;
} drp_merge_report;

int drp_store_merge_report_device(drp_ctx *ctx, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                                  const drp_frames *frames, const drp_changes *cols, uint64_t n,
                                  const drp_filter *filter, const drp_merge_report *report);
/* drp_store_merge_staged (the same rows, return codes and store) that also keeps the merge's news
 * column, with DRP_REPORT_KEEP_BLOBS, in a device buffer of the ctx for the call below. */
int drp_store_merge_news_staged(drp_ctx *ctx, const drp_store *s, const drp_filter *filter, drp_store_info *info_host);
/* drp_fanout_staged with that column in the staged type column's place: the same outputs, splice
 * numbering and DRP_E_CAPACITY contract (it can be called again with a larger out; a merge could not
 * be repeated to retry, the second time nothing would be news), the same bytes in every
 * drp_set_blob_skip mode. After a refused merge every output is empty and the blobs are still listed.
 * DRP_E_INVAL: no news is held (before any drp_store_merge_news_staged, after anything that ends the
 * staged batch for drp_fanout_staged, after a new stage); drp_fanout_staged's cases. */
int drp_fanout_news_staged(drp_ctx *ctx, const drp_filter *filters, uint32_t nfilters, uint8_t *out, uint64_t cap,
                           uint64_t *out_off, uint64_t *n_selected, uint64_t *blob_row, uint64_t *blob_pos,
                           uint64_t blob_cap, uint64_t *n_blobs);

/* ---- lookup: a read-only probe of the store by key (multi-get, have-list sync) --------------- */
/* Every call above either writes the store or scans all max_keys rows of it. Two questions a hub is
 * asked all the time need neither: "give me the current Change of these keys" (a multi-get: equality
 * on the identity, not a key prefix, and any number of keys per call), and "here is what I hold, send
 * what I lack" (a peer's have-list: Changes without values, that is identities and versions, which a
 * merge would write into the store in the values' place). The lookup probes the identity table as a
 * merge does and writes nothing into the store. No reference counterpart (the reference has no relay);
 * the fields read are subset, key and change of messages/schema.proto:1-8.
 *   Queries: exactly the candidates of drp_latest_device for (bytes, nbytes, frames, cols, n, filter):
 * the rows drp_select_device selects whose key range, and with DRP_F_SUBSET whose subset range, lies
 * inside [0, nbytes). Every other row is DRP_LOOKUP_NONE and nothing of it is read; the value is
 * never read for any row. frames / cols need not come from a decode: any columns of that layout over
 * any device bytes do (a list of keys laid end to end, type = DRP_TYPE_CHANGE, is a batch of queries).
 *   The identity is the store section's. verdict[r] compares the query's `change` with the store
 * row's, unsigned 64-bit: ABSENT (no row of this identity), BEHIND (the stored change is smaller: the
 * hub lacks the query's), LEVEL (equal), AHEAD (the stored change is greater: the sender lacks the
 * store's row). hit_row[r] is the store row, UINT64_MAX for NONE and ABSENT. counts[code] is the
 * number of rows in [0, n) with that verdict. Queries are independent: the same identity may be
 * queried many times, with different `change`, and each row gets its own verdict; nothing is
 * de-duplicated.
 *   Read-only: no byte of the store changes (the arena, the columns, the table and the info record
 * stay as they were). info is not read: rows are bounded by max_keys, and the table names only rows
 * in use.
 *   Emission, with out_rows: the queries whose verdict's bit is set in emit_mask, in batch-row order
 * (a stable compaction); for each the store's row of that identity, written as drp_select_device
 * writes that row over the store's view: offsets absolute into s->arena, flags masked to DRP_F_SUBSET
 * | DRP_F_VALUE; out_query[j] is the batch row of emitted row j. *n_out always carries the true
 * count; if it exceeds rows_cap nothing is written to the arrays (drp_fanout_device's rows_cap
 * convention), otherwise entries at or beyond it are left untouched. drp_encode_device(ctx, out_rows,
 * s->arena, s->arena_bytes, *n_out, ...) gives the bytes; the offsets hold until the next
 * drp_store_compact. A multi-get is emit_mask = BEHIND | LEVEL | AHEAD; "only if newer than mine" is
 * emit_mask = AHEAD.
 *   lack_type, a replacement for s->frames.type (max_keys entries): lack_type[j] = s->frames.type[j],
 * except 0 where at least one query hit row j with a `change` greater than or equal to the stored
 * one. Rows no query names stay Changes; rows at or beyond info.rows are 0 as in frames.type. So
 * (s->arena, s->arena_bytes, {payload_off, payload_len, lack_type}, &s->cols, max_keys) is a decoded
 * batch holding exactly the store's rows the sender of the have-list lacks: drp_select_device,
 * drp_fanout_device, drp_order_device behind them, drp_digest_device and the encoder run over it
 * unchanged, and no other column is copied. The outcome does not depend on the order of the queries
 * (the only writes after the copy of the type column are zeros). lack_type == s->frames.type
 * (aliasing) is DRP_E_INVAL.
 *   Entries of verdict / hit_row at or beyond n and of lack_type at or beyond max_keys are left
 * untouched.
 *   Device pointers only; asynchronous on drp_stream(ctx), no host synchronisation inside; the result
 * is a function of the input alone. drp_set_latest_hash_mask applies: a lookup must see the mask the
 * store has seen.
 *   DRP_E_INVAL: drp_store_merge_device's cases; a NULL lk; unknown flags; an emit_mask bit other than
 * those of BEHIND, LEVEL and AHEAD; out_rows without n_out; with rows_cap > 0 a NULL array in
 * out_rows; the aliasing above. (Those of lk are checked before the ctx is used.) Scratch from the
 * ctx's (DRP_E_NOMEM if it cannot be had): 512 bytes of filter strings, 12 bytes per batch row (only
 * with n_out: the emitted queries' store rows and ranks) and 48 bytes per 256 rows (the workgroups'
 * counts). */
#define DRP_LOOKUP_NONE   0 /* the row is no query */
#define DRP_LOOKUP_ABSENT 1 /* the store holds no row of this identity */
#define DRP_LOOKUP_BEHIND 2 /* it does, with a smaller `change` than the query's (the hub lacks the query's) */
#define DRP_LOOKUP_LEVEL  3 /* equal `change` */
#define DRP_LOOKUP_AHEAD  4 /* the store's `change` is greater (the sender lacks the store's row) */
#define DRP_LOOKUP_BIT(code) (1u << (code))

typedef struct drp_lookup { /* HOST struct of DEVICE pointers, read before the call returns; 88 bytes */
  uint32_t flags;     /* 0 (unknown bits: DRP_E_INVAL) */
  uint32_t emit_mask; /* DRP_LOOKUP_BIT of BEHIND / LEVEL / AHEAD; any other bit: DRP_E_INVAL */
  uint8_t *verdict;   /* n entries, may be NULL */
  uint64_t *hit_row;  /* n entries, may be NULL: the store row, UINT64_MAX for NONE and ABSENT */
  uint64_t *counts;   /* 5 entries, may be NULL: rows [0, n) per verdict code */
  uint8_t *lack_type; /* max_keys entries, may be NULL */
  const drp_change_src *out_rows; /* HOST pointer to a struct of writable device arrays, rows_cap entries each; NULL: no emission */
  uint64_t *out_query; /* rows_cap entries, may be NULL: the batch row of each emitted row */
  uint64_t *n_out;     /* one entry; required with out_rows */
  uint64_t rows_cap;
  uint64_t reserved;
  uint64_t reserved2; /* neither is read */
} drp_lookup;

int drp_store_lookup_device(drp_ctx *ctx, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                            const drp_frames *frames, const drp_changes *cols, uint64_t n,
                            const drp_filter *filter, const drp_lookup *lk);
/* That lookup over the delivered rows of the batch last staged (the rows, validity rules and
 * DRP_E_INVAL cases of drp_latest_staged; `filter` says which of them are queries; the same bytes in
 * every drp_set_blob_skip mode), and its reply, encoded with the arena as the heap. reply is an emit_mask: the emitted rows, in batch-row
 * order; or DRP_LOOKUP_REPLY_LACK alone: every store row under lack_type, in store-row order
 * (drp_select_device with a NULL filter over that view; the column lives in a buffer of the ctx).
 * Any other value is DRP_E_INVAL. Synchronous; out is a host or device pointer; *n_rows is the
 * reply's rows, counts_host (HOST, 5 entries, may be NULL) receives the verdict counts. DRP_E_CAPACITY
 * as drp_relay_staged: *written is the size needed and nothing is written to out. The staged batch
 * stays valid. */
#define DRP_LOOKUP_REPLY_LACK 0x100u
int drp_store_lookup_staged(drp_ctx *ctx, const drp_store *s, const drp_filter *filter, uint32_t reply,
                            uint8_t *out, uint64_t cap, uint64_t *written, uint64_t *n_rows,
                            uint64_t *counts_host /* 5, may be NULL */);

/* ---- store lifecycle: load distinct rows, rehash (grow, prune, restore) ----------------------- */
/* A store's max_keys and table are fixed at drp_store_init, its rows keep their index, and its table
 * is a product of the merges that filled it. Growing it, dropping rows from it and bringing it back
 * from saved columns all come down to two calls: enter rows that are known to be new, without the
 * grouping and the lookup a merge pays for, and rebuild the table from the rows. No reference
 * counterpart (the reference has no relay).
 *   drp_store_load_device. The arguments and DRP_E_INVAL cases are drp_store_merge_device's. Loaded
 * rows: exactly the rows drp_select_device selects for (bytes, nbytes, frames, cols, n, filter), in row
 * order; with the store's view as the batch, a type column of the caller's in frames->type's place
 * (a lookup's lack_type, a report's news_type, the store's own with entries zeroed) says which rows.
 *   Precondition, the caller's promise: the loaded rows' identities are pairwise distinct and none is
 * in the store. Nothing is grouped, looked up or compared.
 *   A loaded row is `skipped`, counted and never read, if its key range, its subset range (with
 * DRP_F_SUBSET) or its value range (with DRP_F_VALUE) leaves [0, nbytes), or its three lengths sum
 * past 2^32 - 16. Every other row is `inserted` exactly as a merge inserts: as row info.rows + its rank
 * among the inserted in row order, in the stored form above, its payload at arena_used + the
 * 16-rounded sizes of the inserted before it.
 *   All or nothing, by the merge's verdict: refused, need_rows, need_bytes. The record's last-merge
 * group: winners = the selected rows, inserted, skipped, and replaced = unchanged = stale = 0. merges
 * is counted unless the load is refused.
 *   clash (DEVICE, one entry, may be NULL: then the check does not run): after the rows are written,
 * every loaded row probes the table for its own identity; *clash is the number of rows for which the
 * probe names another row. That is the loaded rows minus the new distinct identities among them: a
 * function of the input alone, and 0 exactly when the precondition held (0 after a refused load).
 * With *clash > 0 the store holds two rows of one identity and every later merge or lookup of it may
 * meet either: the store must be dropped. The call is meant for a store the caller is building
 * (Store.retain in drp_amd.py loads into a fresh one and keeps the old one on a clash).
 *   Device pointers only; asynchronous on drp_stream(ctx), no host synchronisation inside. Scratch from
 * the ctx's (DRP_E_NOMEM if it cannot be had): drp_select_device's, and per row of the batch 80 bytes
 * of selected rows and 32 bytes of merge state. There is no grouping table; a caller bounds the
 * scratch by loading in pieces (a load into a store that holds rows appends). */
int drp_store_load_device(drp_ctx *ctx, const drp_store *s, const uint8_t *bytes, uint64_t nbytes,
                          const drp_frames *frames, const drp_changes *cols, uint64_t n,
                          const drp_filter *filter, uint64_t *clash /* device, 1 entry, may be NULL */);
/* Rebuild the table from the rows: s->table (drp_store_table_bytes(max_keys) bytes) is zeroed and the
 * rows [0, min(info.rows, max_keys)) (info.rows is read on the device) are entered under the ctx's
 * current hash mask, each from its home slot forward as a merge's inserted winner is. The arena, the
 * columns and rows / arena_used / arena_dead / merges of the record are not written; the last-merge
 * group is zeroed. A row whose payload range [payload_off, payload_off + payload_len) leaves
 * [0, arena_bytes), or whose key_len + subset_len exceeds payload_len, is never read and not entered:
 * no lookup or merge finds it.
 *   report (DEVICE, two entries, may be NULL: then the check does not run): report[0] = the rows not
 * entered; report[1] = the entered rows whose probe for their own identity names another row (the
 * load's check over all rows: the rows minus the distinct identities). refused = 1 if either is
 * nonzero, else 0.
 *   After a rehash the store's hash mask is the ctx's current one: the "one mask for its whole life"
 * rule above starts again there.
 *   Restore: upload the columns, the arena and the record, then rehash. Grow without a payload copy:
 * larger columns and a larger table, the old columns copied, frames.type zero beyond them, then
 * rehash. DRP_E_INVAL: drp_store_init's cases. Asynchronous on drp_stream(ctx); no scratch. */
int drp_store_rehash_device(drp_ctx *ctx, const drp_store *s, uint64_t *report /* device, 2 entries, may be NULL */);

/* ---- ordered catch-up: a fan-out's outputs in `change` order, with a per-peer limit ---------- */
/* Every output of the select, fan-out and latest calls above is in row order; over a store that is
 * the order in which identities first entered. A peer names its position in a feed by one number,
 * its version T, so a catch-up it can resume ("I have everything up to T'") or take in pages ("the
 * next M changes after T") must reach it in `change` order. The call below sits between a fan-out
 * and the encode. No reference counterpart (the reference has no relay); the field read is `change`
 * of messages/schema.proto:1-8.
 *   Order: output segment f holds the rows of input segment f in ascending `change`, compared as
 * unsigned 64-bit; rows of equal `change` keep their input order (after a fan-out: source row order).
 *   Limit: limit is a HOST array of nseg entries, read before the call returns (NULL, or an entry of
 * UINT64_MAX: no limit). With cnt_f = row_base[f + 1] - row_base[f], output f keeps the first
 * min(cnt_f, limit[f]) rows of that order. With DRP_ORDER_KEEP_TIES a cut that falls inside a run of
 * equal `change` moves forward to the end of the run: the output may then exceed the limit, never
 * cnt_f, a limit of 0 still keeps nothing, and a peer that resumes with change > the last change
 * sent loses no row and every page makes progress. Without the flag the cut is exact. */
#define DRP_ORDER_KEEP_TIES 0x01
/* rows: encoder rows (rows_cap entries per array) and row_base (device, nseg + 1 entries) as
 * drp_fanout_device and drp_fanout_latest_device leave them: segment f is rows [row_base[f],
 * row_base[f + 1]). out_rows: a second, caller-owned set of rows_cap entries per array; out_base
 * (device, nseg + 1 entries): out_base[0] = 0, out_base[f + 1] = out_base[f] + the rows output f
 * keeps, so the outputs lie end to end and one drp_encode_device over out_base[nseg] rows encodes
 * every peer's page. out_sel_idx (may be NULL; needs sel_idx) receives sel_idx in the same order.
 * Entries of out_rows and out_sel_idx at or beyond out_base[nseg] are left untouched. Not a valid
 * input: row_base[nseg] > rows_cap (the fan-out wrote no rows then), or a row_base that is not
 * non-decreasing; out_base[0 .. nseg] is then all 0 and out_rows and out_sel_idx are left untouched.
 * The result is a function of the input alone. Device pointers only; asynchronous on
 * drp_stream(ctx), no host synchronisation inside (the counts are read on the device).
 * DRP_E_INVAL: nseg 0 or above DRP_FANOUT_MAX; a NULL rows, row_base, out_rows or out_base (or, with
 * rows_cap > 0, a NULL array in rows or out_rows); out_sel_idx without sel_idx; out_rows->change ==
 * rows->change (no in-place sort); unknown flag bits; rows_cap above 2^32 - 1 (row indices are
 * 32-bit inside). Scratch, from the ctx's (DRP_E_NOMEM if it cannot be had): 24 bytes per entry of
 * rows_cap, and about 1 KiB per 4096 entries. */
int drp_order_device(drp_ctx *ctx, const drp_change_src *rows, const uint64_t *row_base, uint32_t nseg,
                     uint64_t rows_cap, const uint64_t *limit, uint32_t flags, const drp_change_src *out_rows,
                     const uint64_t *sel_idx, uint64_t *out_sel_idx, uint64_t *out_base);

/* ---- key-ordered listing: a fan-out's outputs in key order, with a key range and a page -------- */
/* Row order and `change` order mean nothing to a client that iterates a key/value store: "list what
 * is under users/, 500 at a time, resuming after the last key I saw", "give me the range [a, m)",
 * "export this subset in a stable order" need the rows in key order. The call below sits where
 * drp_order_device does, between a fan-out and the encode, and takes the same rows; the listing's
 * subset, key prefix and version bound are the fan-out's ordinary filters. No reference counterpart
 * (the reference has no relay); the fields read are `key` and `subset` of messages/schema.proto:1-8.
 *   Input and output shape: rows, row_base, nseg, rows_cap, out_rows, sel_idx, out_sel_idx and out_base
 * are exactly drp_order_device's, with its rule for an input that is not valid (out_base all 0,
 * nothing else written; totals, if given, {0, 0}) and its rule that entries of out_rows and
 * out_sel_idx at or beyond out_base[nseg] are left untouched. heap / heap_bytes (device) is what the
 * rows' offsets are absolute into: the wire of a decoded batch, or a store's arena.
 *   Order: within a segment ascending by the tuple (key bytes; subset presence, absent first; subset
 * bytes; input position). Byte strings compare as unsigned bytes, lexicographically, a proper prefix
 * first: "ab" < "ab\0" < "ab\0\0" < "ab\x01", and 0x7F < 0x80 < 0xFF. The key is the major field, so
 * a key range is one contiguous run of the sorted segment.
 *   Rows left out: a row whose key range [key_off, key_off + key_len) leaves [0, heap_bytes), or,
 * with DRP_F_SUBSET, whose subset range does, or whose key or (with DRP_F_SUBSET) subset is longer
 * than DRP_KEYORDER_MAX_BYTES, is never read, is in no output and is counted in totals[1]; totals[0]
 * counts the rows that took part (totals: device, 2 entries, may be NULL). No byte at or beyond heap +
 * heap_bytes is read, not even as the padding of a word.
 *   Range: pages is a HOST array of nseg entries, and so are the lo / hi bytes it points to; all are
 * read before the call returns. Segment f keeps the rows of its sorted order whose key lies inside
 * pages[f]'s bounds: FROM key >= lo, AFTER key > lo (a resume cursor), UNTIL key < hi. The bounds apply
 * to the key only; an empty bound is a bound (lo or hi may be NULL when its length is 0); lo >= hi
 * keeps nothing. A NULL pages, or flags == 0 with limit == UINT64_MAX, keeps everything.
 *   Limit: of the kept run, segment f keeps the first min(count, limit) rows. With
 * DRP_KEYORDER_KEEP_TIES a cut inside a run of equal key (the same key bytes; the subsets may differ)
 * moves forward to the end of that run: the output may then exceed the limit, never the run, a limit
 * of 0 still keeps nothing, and a peer that resumes with AFTER = the last key sent loses no row and
 * every non-empty page makes progress. Without the flag the cut is exact. */
#define DRP_KEYORDER_KEEP_TIES 0x01
#define DRP_KEYORDER_MAX_BYTES 4096 /* longest key / subset that takes part, longest bound */

#define DRP_KEYPAGE_FROM  0x01 /* keep key >= lo */
#define DRP_KEYPAGE_AFTER 0x02 /* keep key >  lo  (a resume cursor); with FROM: DRP_E_INVAL */
#define DRP_KEYPAGE_UNTIL 0x04 /* keep key <  hi */
typedef struct drp_key_page {   /* HOST, one per segment; lo / hi HOST too, read before the call returns */
  uint32_t flags, lo_len, hi_len, reserved;
  const uint8_t *lo, *hi;       /* may be NULL when the length is 0 (an empty bound is a bound) */
  uint64_t limit;               /* UINT64_MAX: none */
} drp_key_page;
/* The result is a function of the input alone. Device pointers only (but pages and its bounds), on
 * drp_stream(ctx). Host waits: exactly one. After a first pass over the rows the call waits for the
 * stream to read 32 bytes (the longest key and subset that take part, the counts), which size the
 * launch chain: one run of the sort's digit passes per 8-byte word of the longest key and of the
 * longest subset, and none for a field no row has. Which digits of a word run is decided on the
 * device, as in drp_order_device, without a further wait; everything after the wait is asynchronous.
 * DRP_E_INVAL: every case of drp_order_device (nseg 0 or above DRP_FANOUT_MAX; a NULL rows, row_base,
 * out_rows or out_base, or, with rows_cap > 0, a NULL array in rows or out_rows; out_sel_idx without
 * sel_idx; out_rows->change == rows->change; rows_cap above 2^32 - 1); a NULL heap with heap_bytes >
 * 0; unknown bits in flags or in a page's flags; FROM together with AFTER; a bound longer than
 * DRP_KEYORDER_MAX_BYTES; a NULL bound with a nonzero length. All of these are reported before the
 * ctx is touched. Scratch, from the ctx's (DRP_E_NOMEM if it cannot be had): drp_order_device's (24
 * bytes per entry of rows_cap, about 1 KiB per 4096 entries), one more byte per entry, 1 KiB, and the
 * bounds' bytes (at most 8 KiB per segment). */
int drp_order_keys_device(drp_ctx *ctx, const uint8_t *heap, uint64_t heap_bytes,
                          const drp_change_src *rows, const uint64_t *row_base, uint32_t nseg,
                          uint64_t rows_cap, const drp_key_page *pages /* nseg, may be NULL */,
                          uint32_t flags, const drp_change_src *out_rows, const uint64_t *sel_idx,
                          uint64_t *out_sel_idx, uint64_t *out_base, uint64_t *totals /* device, 2, may be NULL */);

/* ---- digest / reconcile: what differs between two stores, without a shared version ---------- */
/* "What changed since T?" needs two parties that share one `change` counter. Two hubs that each hold
 * a store, or a hub that merges several peers' feeds, have none; they compare content instead: a
 * digest of the rows per bucket of identities (16 bytes a bucket), a diff of two digests, and a select
 * that keeps the rows of the differing buckets, which one drp_encode_device then sends and the peer's
 * drp_store_merge_device takes in. No reference counterpart (the reference has no relay); the fields
 * read are those of messages/schema.proto:1-8.
 *   The digest crosses the network, so it is defined bit for bit. All arithmetic is modulo 2^64;
 * XXH64 is the published function with seed 0, P1 .. P4 its primes, rotl a left rotation:
 *     merge(a, v)  = (a ^ (rotl(v * P2, 31) * P1)) * P1 + P4
 *     avalanche(h) : h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32
 *     ident(row)   = XXH64(key); with DRP_F_SUBSET: ident = merge(ident, XXH64(subset))
 *                    (an empty subset still merges: the identity of drp_latest_device and the store)
 *     fp(row)      = ident; for v in (change, from, to, flags & (DRP_F_SUBSET | DRP_F_VALUE)):
 *                    fp = merge(fp, v); with DRP_F_VALUE: fp = merge(fp, XXH64(value)) (an empty value
 *                    still merges); fp = avalanche(fp)
 *     bucket(row)  = bits ? ident >> (64 - bits) : 0
 *     cell[b]      = { count: the rows of bucket b, sum: the sum of their fp }
 * fp covers what the store's `unchanged` rule compares. drp_set_latest_hash_mask does not reach any
 * of this: it is a hook of the grouping tables only.
 *   Candidates: the rows drp_select_device selects under the filter (NULL or flags == 0: every
 * well-formed Change) whose key range, with DRP_F_SUBSET subset range and with DRP_F_VALUE value
 * range lie inside [0, nbytes). A selected row with a range that leaves the wire is never read and is
 * in no cell; it is counted in totals[1].
 *   The digest is over the rows as they stand: over a store's view or drp_latest_device's output,
 * where identities are distinct, the cells are a function of the set of (identity, content); over a
 * raw batch a row that occurs twice counts twice. The order of the rows never matters.
 *   Limit: two stores converge under mutual reconcile-and-merge only if no identity carries two
 * different contents at the same `change` (a log never does). With such a pair each side would take
 * the other's row, by the store's "equal change, later arrival wins" rule, and they would swap. */
#define DRP_DIGEST_MAX_BITS 16
typedef struct drp_digest_cell {
  uint64_t count, sum;
} drp_digest_cell;

/* The digest of the candidates among decoded rows [0, n): cells (device, 2^bits entries) is zeroed
 * and filled; totals (device, two entries, may be NULL): [0] the rows digested, [1] the selected rows
 * left out for a range outside the wire. bytes, frames, cols, n and filter follow drp_latest_device's
 * argument rules (out_rows aside) and DRP_E_INVAL cases; a store's view (s->arena, s->arena_bytes,
 * &s->frames, &s->cols, n = max_keys) is a valid input. DRP_E_INVAL also for bits >
 * DRP_DIGEST_MAX_BITS and NULL cells. Device pointers only; asynchronous on drp_stream(ctx), no host
 * synchronisation inside. The result is a function of the input alone. Scratch from the ctx's: 512
 * bytes (the filter's byte strings). */
int drp_digest_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                      const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                      drp_digest_cell *cells, uint64_t *totals);
/* Two digests of 2^bits cells each (a, b: device) compared: bucket_set (device, max(1, 2^bits / 64)
 * words) gets bit b & 63 of word b >> 6 set iff a[b] and b[b] differ in count or sum; the unused high
 * bits of the one word of bits < 6 are 0. *n_diff (device) = the bits set. Asynchronous on
 * drp_stream(ctx); no scratch. DRP_E_INVAL: a NULL pointer, bits > DRP_DIGEST_MAX_BITS. */
int drp_digest_diff_device(drp_ctx *ctx, const drp_digest_cell *a, const drp_digest_cell *b, uint32_t bits,
                           uint64_t *bucket_set, uint64_t *n_diff);
/* drp_select_device restricted to the digest's candidates whose bucket's bit is set in bucket_set
 * (device, as drp_digest_diff_device writes it): the same stable compaction and the same out_rows,
 * sel_idx and n_selected contract. Under one filter and one bits, the rows kept are exactly the rows
 * drp_digest_device counted in the cells of the set buckets. The argument rules and DRP_E_INVAL cases
 * are drp_select_device's, and bits > DRP_DIGEST_MAX_BITS or a NULL bucket_set. Asynchronous on
 * drp_stream(ctx). Scratch from the ctx's: drp_select_device's (one bit per row, 8 bytes per 1024
 * rows, 512 bytes). */
int drp_select_buckets_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                              const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                              const uint64_t *bucket_set, const drp_change_src *out_rows, uint64_t *sel_idx,
                              uint64_t *n_selected);

/* ---- refined digests: a second level inside the differing buckets --------------------------- */
/* At DRP_DIGEST_MAX_BITS a bucket of a large store still holds many keys, and one altered key sends
 * them all; a dense digest of more bits would outweigh the snapshot. The second level is sparse: cells
 * only for the buckets of a set (the buckets in which the first-level digests differ), addressed by
 * the next sub_bits bits of the same identity hash. Both hubs hold both first-level digests, so both
 * derive the same bucket_set; each sends its second-level cells, and each then sends the rows of the
 * cells that differ. No reference counterpart.
 *   Defined bit for bit, as the first level is. ident, fp, the candidates and bucket(row) are those of
 * the section above; bucket_set is the bit set drp_digest_diff_device writes for `bits`;
 * 1 <= sub_bits <= DRP_DIGEST_MAX_SUB_BITS:
 *     slot(b)    = the number of set bits of bucket_set below bit b        (only for a set b)
 *     sub(row)   = (ident >> (64 - bits - sub_bits)) & (2^sub_bits - 1)    (bits = 0: ident >> (64 - sub_bits))
 *     cell2(row) = slot(bucket(row)) * 2^sub_bits + sub(row)
 *     n_set      = the set bits of bucket_set;   ncells = n_set << sub_bits
 *     cells2[c]  = { count, sum of fp } of the candidates whose bucket is set and whose cell2 is c
 * Consequence: the 2^sub_bits cells of slot s add up (count and sum, modulo 2^64) to the first-level
 * cell of the s-th set bucket. With bits < 6 only the low 2^bits bits of the one word name buckets. */
#define DRP_DIGEST_MAX_SUB_BITS 8

/* The second-level cells of the candidates among decoded rows [0, n) whose bucket's bit is set in
 * bucket_set (device, max(1, 2^bits / 64) words). totals (device, three entries, required): [0] the
 * rows digested (the candidates in set buckets), [1] the selected rows left out for a range outside
 * the wire (drp_digest_device's count, whatever the set), [2] n_set. If ncells <= cells_cap,
 * cells2[0, ncells) (device) is zeroed and filled and the entries from ncells on are left untouched;
 * otherwise nothing is written to cells2 and totals is still complete (drp_fanout_device's rows_cap
 * convention). With n_set == 0 nothing is written to cells2. Of a candidate outside the set buckets
 * only the key and subset bytes are read, never the value. The other arguments and DRP_E_INVAL cases
 * are drp_digest_device's, and sub_bits of 0 or above DRP_DIGEST_MAX_SUB_BITS, a NULL bucket_set,
 * cells2 or totals. Device pointers only; asynchronous on drp_stream(ctx), no host synchronisation
 * inside; the result is a function of the input alone. Scratch from the ctx's: the filter's 512
 * bytes and a rank table of 4 bytes per word of bucket_set. */
int drp_digest_refine_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                             const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                             const uint64_t *bucket_set, uint32_t sub_bits, drp_digest_cell *cells2,
                             uint64_t cells_cap, uint64_t *totals);
/* drp_digest_diff_device for any cell count (a host number, at most 65536 << 8; the caller has n_set
 * on the host by now, it sizes what it sends from it): cell_set (device, max(1, ceil(ncells / 64))
 * words) gets bit c set iff a[c] and b[c] differ in count or sum, the unused high bits of the last
 * word are 0; *n_diff (device) = the bits set. ncells == 0: *n_diff = 0 and the one word is 0.
 * Asynchronous on drp_stream(ctx); no scratch. DRP_E_INVAL: a NULL pointer, ncells above the most. */
int drp_digest_diff_cells_device(drp_ctx *ctx, const drp_digest_cell *a, const drp_digest_cell *b, uint64_t ncells,
                                 uint64_t *cell_set, uint64_t *n_diff);
/* drp_select_buckets_device with the further condition that bit cell2(row) of cell_set (device, as
 * drp_digest_diff_cells_device writes it for ncells) is set: the same stable compaction and the same
 * out_rows, sel_idx and n_selected contract. Under one filter, bits, bucket_set and sub_bits the rows
 * kept are exactly the rows drp_digest_refine_device counted in the set cells. DRP_E_INVAL cases:
 * drp_select_buckets_device's, and sub_bits of 0 or above DRP_DIGEST_MAX_SUB_BITS or a NULL cell_set.
 * Asynchronous on drp_stream(ctx). Scratch from the ctx's: drp_select_device's and the rank table. */
int drp_select_refined_device(drp_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const drp_frames *frames,
                              const drp_changes *cols, uint64_t n, const drp_filter *filter, uint32_t bits,
                              const uint64_t *bucket_set, uint32_t sub_bits, const uint64_t *cell_set,
                              const drp_change_src *out_rows, uint64_t *sel_idx, uint64_t *n_selected);

/* ---- multi-GPU global index ---------------------------------------------- */
/* stats[nranks*per_rank] (device): all-gathered per-stream tables in rank order.
 * Writes base[nranks*per_rank] (device): exclusive prefix of frames = global index of
 * each stream's first frame. Asynchronous. */
int drp_index_scan(drp_ctx *ctx, const drp_stream_stats *stats, uint64_t count, uint64_t *base);
/* results[nstreams] (device) -> stats[nstreams] (device), asynchronous. */
int drp_stream_stats_from_results(drp_ctx *ctx, const drp_stream_result *results,
                                  const uint64_t *stream_off, uint64_t nstreams,
                                  drp_stream_stats *stats);

/* ---- multi-GPU all-gather over RCCL ----------------------- */
/* The only collective of the codec: independent streams are sharded across GPUs (contiguous
 * blocks of stream ids), each GPU decodes its block (drp_decode_device) and builds its stats
 * (drp_stream_stats_from_results); the records are all-gathered (ncclAllGather over xGMI)
 * and scanned on every GPU into the global index of each stream's first frame.
 * No reference counterpart (the reference is one stream on one thread). */
#define DRP_COMM_ID_BYTES 128
typedef struct drp_comm drp_comm;
/* One process per GPU: rank 0 creates the id (ncclGetUniqueId), the launcher hands the bytes
 * to every rank, each rank joins with its ctx. */
int drp_comm_id(uint8_t *id /* [DRP_COMM_ID_BYTES] */);
int drp_comm_init_rank(drp_ctx *ctx, const uint8_t *id, int nranks, int rank, drp_comm **out);
/* One process driving ngpu devices: one comm per ctx (ncclCommInitAll). */
int drp_comm_init_all(drp_ctx **ctxs, int ngpu, drp_comm **comms);
void drp_comm_destroy(drp_comm *comm);
/* local[per_rank] -> global[nranks * per_rank] (rank order) and base[nranks * per_rank]: the
 * exclusive prefix of frames = the global index of every stream's first frame (a short block
 * is padded with zero records). Device pointers; returns after completion. */
int drp_index_allgather(drp_ctx *ctx, drp_comm *comm, const drp_stream_stats *local, uint64_t per_rank,
                        drp_stream_stats *global, uint64_t *base);
/* The same for ngpu contexts in one process (one grouped all-gather). */
int drp_index_allgather_multi(drp_ctx **ctxs, drp_comm **comms, int ngpu, const drp_stream_stats *const *local,
                              uint64_t per_gpu, drp_stream_stats *const *global, uint64_t *const *base);
/* drp_index_allgather_multi from HOST arrays (a host that keeps its per-stream counters on the
 * CPU, e.g. the N-API addon): local[g][per_gpu] are staged to device g, all-gathered over RCCL,
 * scanned on every device, and device 0's table and bases are copied to global[ngpu * per_gpu]
 * and base[ngpu * per_gpu]. Returns after completion. */
int drp_index_allgather_host(drp_ctx **ctxs, drp_comm **comms, int ngpu, const drp_stream_stats *const *local,
                             uint64_t per_gpu, drp_stream_stats *global, uint64_t *base);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DRP_H */
