// drp_kernels.h — parameter blocks and launchers shared by the kernels and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/drp.h"

namespace drp {

// sizes of scratch regions and staged columns: up to the next multiple of 256 bytes
inline uint64_t al(uint64_t x) { return (x + 255) & ~255ull; }

struct DecodeParams {
  const uint8_t *bytes;
  uint64_t nbytes;
  const uint64_t *stream_off;
  const uint64_t *entry;
  uint64_t nstreams;
  const uint64_t *tile_prefix;  // [nstreams+1]
  // outputs
  uint64_t *payload_off;
  uint32_t *payload_len;
  uint8_t *type;
  uint32_t *key_off, *key_len, *subset_off, *subset_len, *value_off, *value_len;
  uint64_t *change, *from, *to;
  uint8_t *flags;
  uint64_t cap;
  // per-tile look-back words (value + 1, or READY-tagged; 0 = not yet published)
  uint64_t *ywd;    // Y_t: <= 3 distinct exits landing in tile t+1 (16-bit rel + 1) | READY
  uint64_t *aggv;   // agg_t: f_t on the slots of Y_{t-1} (16-bit codes) | READY
  uint64_t *aggn;   // frames delivered by tile t on each of those paths (16-bit) | READY
  uint64_t *inclx;  // exact exit of tile t + 1
  uint64_t *aggc;   // delivered frames of tile t + 1
  uint64_t *inclc;  // frames of tiles <= t + 1
  uint64_t *tile_exit, *tile_base, *tile_count;  // per-tile records for finalize
  // per super-group (64 tiles): completion counters, composed map, count sum (value + 1)
  uint32_t *sgc_agg, *sgc_cnt;
  uint64_t *sagg, *saggn, *scnt;  // saggn: 20-bit frame counts per key
  // per-stream scratch
  uint64_t *payload_err;  // min absolute index of a malformed Change
  uint64_t *scount;       // [2*s] changes, [2*s+1] blobs
  // control
  uint32_t *counter;
  uint32_t *overflow;  // bit 0 capacity, bit 1 bounded wait expired, bit 2 inconsistent walk
  uint32_t strict;     // look-back uses exact inclusive exits only (test hook)
  // speculate-and-verify kernel (drp_decode_spec.hip): per-tile words, value | READY or value + 1
  uint64_t *claim;     // predicted exit of tile t (or identity)
  uint64_t *incl_e;    // entry of tile t + 1
  uint64_t *agg_n;     // exact frames of tile t + 1
  uint64_t *incl_n;    // frames of tiles <= t + 1
  const uint32_t *tile_stream;  // tile -> stream (null: one stream; drp_launch_spec_head fills it)
  uint8_t *ent;                 // [tile][thread]: entry offset in the thread's 64 B, 0xFF none
  uint8_t *ent_n, *ent_c;       // [tile][thread]: frames / change frames from that entry
  uint32_t *work;               // tiles for the general claims kernel (edge / dense tiles)
  uint32_t *work_n;             //  and their count (the fast claims kernel appends)
  uint64_t *tile_nch;           // change frames of tile t (per-stream counts come from a scan:
  uint64_t *tile_nch_base;      //  same-address atomics per tile serialise across the XCDs)
  // verify_lite: tiles it leaves to verify_counts, and each tile's first entry thread (emit skips
  // the threads before it); null: verify_counts verifies every tile
  // (the host always sets vlist: the kernels' null forms are kept only so their code does not change)
  uint32_t *vlist, *vlist_n;
  uint8_t *tile_k;
  // per tile: 1 when the tile is sparse (every thread from tile_k on delivers at most one frame,
  // at its entry; a few frames in all): emit_sparse decodes its frames from HBM without staging
  // the tile, and emit_tiles skips it (emit_sparse clears the mark of a tile it cannot take)
  uint8_t *tile_sparse;
  uint64_t *first_miss;  // per stream: the first tile a verify pass repaired (~0: none)
  // verify_counts appends the tiles whose entry a repair changed (the next repair pass verifies
  // only those); a count past dlist_cap or a nonzero dlist_n[2] means the next pass must be a
  // full one
  uint32_t *dlist, *dlist_n;
  uint64_t dlist_cap;
  uint32_t *vlist_ovf;  // vlist is a dirty list: its overflow word (set: pass the overflow on, verify nothing)
  uint32_t *dstamp;     // per tile: the last pass id whose dirty list holds it (one entry per tile per list)
  uint32_t pass_id;     // this verify pass (1: the head's; zeroed stamps before it)
  uint32_t change_checks;  // 1: claims_fast checks long frames' Change structure (drp_api.hip picks)
  int kstrong_hbm;      // 0: DRP_KSTRONG_HBM; else frames a deferred candidate must survive (tests)
  uint32_t cascade_min;  // listed tiles that make the head's verify a cascade (drp_decode_spec.hip)
  uint32_t jump_min;     // claims tiles whose link rounds hit DRP_FL_CAP before the rest take the
                         // pointer-jumping form (counted in counter[12]; drp_decode_spec.hip)
  // region walkers (drp_walk.hip): per-stream region prefix [nstreams + 1], tiles per region
  uint64_t *walk_rp;
  uint64_t *walk_entry;  // region walkers: each region's entry (walk_sync)
  uint32_t walk_hop;      // 1: the hop walkers (claims_hop), 2: by walk_dense (hop walkers or claims_fast)
  unsigned long long *walk_dense;  // walk_density's sample: bytes, frames after stream entries
  uint32_t walk_tpr;
  // claims_fast's per-frame records (null: none): CR_TILE_WORDS words per tile; per tile REC_NONE
  // (no records: the tile takes the wire-reading emission) or 0, and verification's verdict for the
  // record emission (0: not, else 1 + the slot of the tile's first row)
  uint32_t *rec;
  uint32_t *tile_rec;
  uint8_t *tile_recok;
  uint32_t *chunk_tile;  // per 64 output rows: the tile holding the first (emit_recs' aligned row chunks)
  unsigned long long *stats;  // optional event counters (DRP_STATS=1), see drp_decode.hip
  unsigned long long *trace;  // optional per-tile timestamps (DRP_TRACE_FILE, with DRP_STATS)
};

struct EncodeParams {
  drp_change_src src;
  const uint8_t *heap;
  uint64_t heap_bytes;  // rows whose key/subset/value range leaves [0, heap_bytes) are rejected
  uint64_t n;
  uint64_t *frame_off;  // [n+1] exclusive prefix of frame sizes (written)
  uint8_t *out;
  uint64_t cap;
  uint64_t *block_sum;  // per-block partial sums (scan scratch)
  uint32_t *overflow;  // bit 0 output capacity, bit 1 a row's heap range is out of bounds
  // output-stationary write (enc_write_os): per output block of ENC_BS bytes the first frame whose
  // bytes it holds, the blocks left to the per-frame writer (more frames than fit its LDS), count
  uint64_t *oblk_first;
  uint32_t *dense;
  uint32_t *dense_n;
  uint64_t nob;  // output blocks the grid covers (from cap)
};

// The relay kernels (drp_select.hip, drp_latest.hip, drp_fanout.hip) share their row source, their
// row destination and their filter record; drp_select.h holds the device code over them.
// The decoded rows and the wire their columns point into
struct RowSrc {
  const uint8_t *bytes;
  uint64_t nbytes;
  const uint64_t *payload_off;
  const uint8_t *type;
  drp_changes cols;  // (read only)
  uint64_t n;
  // rows of a batch staged in pieces: piece k holds rows [piece_row[k], piece_row[k + 1]) and its
  // payload offsets are piece_shift[k] short of offsets into `bytes` (npieces <= 1: shift0 for all)
  const uint64_t *piece_row, *piece_shift;
  uint64_t npieces, shift0;
};

// encoder rows (drp_change_src, offsets absolute into the wire) and each one's source row
struct RowOut {
  uint64_t *o_key_off, *o_subset_off, *o_value_off;
  uint32_t *o_key_len, *o_subset_len, *o_value_len;
  uint64_t *o_change, *o_from, *o_to;
  uint8_t *o_flags;
  uint64_t *sel_idx;  // may be null
};

// one filter (drp_filter without its pointers; conditions that are off hold neutral values)
struct RowFilter {
  uint32_t flags, subset_len, prefix_len, reserved;
  uint64_t change_min, change_max;
};
static_assert(sizeof(RowFilter) == 32, "the fan-out's device table holds 32-byte records");
// DRP_SEL_SUBSET_EQ / DRP_SEL_KEY_PREFIX where the filter compares such bytes (a non-empty string)
__host__ __device__ inline uint32_t filter_bytes(const RowFilter &F) {
  return ((F.flags & DRP_SEL_SUBSET_EQ) && F.subset_len ? DRP_SEL_SUBSET_EQ : 0u) |
         ((F.flags & DRP_SEL_KEY_PREFIX) && F.prefix_len ? DRP_SEL_KEY_PREFIX : 0u);
}
constexpr uint32_t FAN_FBYTES = 2 * DRP_SEL_MAX_BYTES;  // per filter: subset, then key prefix

// drp_select.hip: predicate + stable compaction of decoded Change rows into encoder rows
struct SelectParams {
  RowSrc src;
  RowFilter f;
  const uint8_t *subset, *prefix;  // its byte strings in device memory, placed by the launcher
  // scratch (placed by the launcher): one ballot word per 64 rows, one count per workgroup
  uint64_t *mask, *block_cnt;
  RowOut out;
  uint64_t *n_selected;
};

// the filter's byte strings as launch arguments: subset, then key prefix
struct SelectBytes {
  uint8_t b[FAN_FBYTES];
};

// drp_latest.hip's grouping table: nslots (a power of two >= 2 n) slots, all zero before the insert
// step. A slot's first word is rep: hash tag | (the row that claimed the slot + 1)
struct LatTable {
  uint64_t *tab;
  uint64_t nslots;
  uint64_t hash_mask;  // ANDed with the row hash before the tag and the start slot are taken (test hook)
  uint64_t tag_mask;   // rep's hash bits: the high 32 when n < 2^32 - 1 (rows fit the low 32), else none
};
// drp_latest.hip: the select's candidates grouped by (subset presence, subset bytes, key bytes) in
// an insert-only open-addressing table, the row with the greatest (change, row) of every group kept
struct LatestParams {
  SelectParams sel;  // the select's parameters: predicate, scratch and outputs as there
  // slots of three words: [0] rep; [1] the greatest change of the group; [2] the greatest row + 1
  // among those that carry it
  LatTable t;
  uint64_t *slot;  // [n] the slot of row i's group, LAT_NONE for a row that is no candidate
};
constexpr uint64_t LAT_NONE = ~0ull;

// drp_fanout.hip: up to DRP_FANOUT_MAX filters over one pass of the decoded rows
struct FanParams {
  RowSrc src;
  uint32_t nfilters;
  uint32_t any_flags;  // the OR of the filters' flags: the columns the count step reads
  uint32_t any_bytes;  // DRP_SEL_SUBSET_EQ / DRP_SEL_KEY_PREFIX: some filter compares such bytes
  const RowFilter *filt;  // [nfilters], device
  const uint8_t *fbytes;  // [nfilters][FAN_FBYTES], device
  // scratch: ballot words [nfilters + 1][nwords] (the last plane: the blob rows), counts
  // [nfilters + 1][nwg] (scanned in place), the sums of every FAN_SCAN counts, the grand total
  uint64_t *mask, *block_cnt, *bsum, *gtotal;
  uint64_t nwg, nwords;
  RowOut out;
  uint64_t rows_cap;
  uint64_t *row_base;  // [nfilters + 1]
  // splice table (fan_splice; blob_row null: none)
  uint64_t *blob_row, *blob_rank, *n_blobs;
  uint64_t blob_cap, row_bias;  // row_bias: added to every blob_row entry (rows the host put first)
};

// drp_latest.hip: latest per key under every filter of a fan-out. The rows some ballot plane keeps
// are grouped once (slots of one word, rep) and the groups numbered densely, in the order of the rows
// that claimed their slots; the planes are then reduced to their winners in passes of up to `pass`
// filters [f0, f0 + nf)
struct FanLatestParams {
  FanParams fan;  // after fan_count: mask and block_cnt are read and rewritten
  LatTable t;
  uint64_t *group;  // [n] the slot of row i's group, then (flat_number) the group's number; LAT_NONE
                    // for a row that is no candidate of any filter
  uint64_t *lead, *lead_base;  // per 64 rows: the ballot of the rows that claimed a slot, and the
                               // number of such rows before these 64
  uint64_t *state;  // [groups <= n][nf][2], zero before a pass: the greatest change that filter f0 + k
                    // keeps in the group, and the greatest row + 1 among those that carry it
  uint32_t f0, nf;
};
// filters per pass by default: the pass state of one group (16 bytes per filter) is one 128-byte line,
// and the state of a batch at most 128 bytes per row (DESIGN.md "Fan-out of latest per key")
constexpr uint32_t FLAT_PASS_DEFAULT = 8;

// drp_store.hip: the store (drp_store of include/drp.h) as the kernels take it. A word of its table
// is hash tag (the high 32 bits) | store row + 1 (max_keys <= 2^31), 0 for a free slot; nslots is a
// power of two >= 2 max_keys, so the table is at most half full
struct StoreDev {
  uint8_t *arena;
  uint64_t arena_bytes;
  uint64_t *payload_off;
  uint32_t *payload_len;
  uint8_t *type;
  drp_changes cols;
  uint64_t max_keys;
  uint64_t *table;
  uint64_t nslots, hash_mask;  // hash_mask: as LatTable's
  drp_store_info *info;
};
constexpr uint64_t ST_TAG = 0xFFFFFFFF00000000ull;
// one merge: the winners drp_launch_latest left (encoder rows, offsets absolute into the wire, and
// their count on the device) and the merge's state, placed by the launcher
struct StoreMerge {
  StoreDev s;
  const uint8_t *bytes;
  uint64_t nbytes;
  drp_change_src w;
  const uint64_t *nw;  // the winners (<= n)
  uint64_t n;          // the batch's rows: what the grids are sized from
  // per winner: the store row (replaced; inserted: the first free slot of its probe, then, from
  // st_claim on, its new row), the identity's hash, the bytes its workgroup's winners before it
  // need, its allocation, and outcome | rank among its workgroup's inserted winners << 8
  uint64_t *where, *hash, *boff;
  uint32_t *alloc, *meta;
  // per workgroup of ST_BLK winners: inserted winners and bytes needed (each scanned in place), and
  // ST_MISC further sums (replaced, unchanged, stale, skipped, dead bytes)
  uint64_t *blk_ins, *blk_bytes, *blk_misc;
  uint64_t nblk;
  uint64_t *ctl;  // [0] the inserted winners, [1] the bytes needed, [2] the dead bytes, [3] the stale winners
};
// the report of one merge (include/drp.h "merge report"), written by the rep_* steps behind st_commit.
// Every output may be null; the two scratch columns are placed by the caller
struct StoreReport {
  uint32_t flags;           // DRP_REPORT_*
  const uint8_t *type;      // the batch's type column (read with DRP_REPORT_KEEP_BLOBS)
  uint8_t *outcome, *news_type;  // [n]
  const uint64_t *src_row;  // per winner: its batch row (drp_launch_latest's sel_idx); with outcome / news_type
  RowOut reply;             // the stale winners' store rows (reply.sel_idx: reply_idx), reply_cap entries
  uint64_t *n_reply, reply_cap;
  uint64_t *blk_stale;      // per workgroup of ST_BLK winners: its stale winners (scanned in place); with n_reply
};
constexpr uint32_t ST_BLK = 256, ST_WAVES = ST_BLK / 64, ST_MISC = 5;
constexpr uint32_t ST_GRP = 16;  // lanes that copy one payload, 16 bytes each per step
// one lookup (include/drp.h "lookup"): the queries are the candidates among sel.src's rows under
// sel's filter; the store is only read. Every output may be null; the state is placed by the launcher
constexpr uint32_t LK_CODES = 5;  // DRP_LOOKUP_NONE .. DRP_LOOKUP_AHEAD
struct StoreLookup {
  StoreDev s;
  SelectParams sel;    // the row source and the predicate (its scratch and outputs are not used)
  uint32_t emit_mask;  // DRP_LOOKUP_BIT of the verdicts whose store rows are emitted
  uint8_t *verdict;    // [n]
  uint64_t *hit_row;   // [n]
  uint64_t *counts;    // [LK_CODES]
  uint8_t *lack_type;  // [max_keys]
  RowOut out;          // the emitted queries' store rows (out.sel_idx: out_query), rows_cap entries
  uint64_t *n_out, rows_cap;
  // per query, only with n_out: its store row, and verdict | rank among its workgroup's emitted
  // queries << 8
  uint64_t *where;
  uint32_t *meta;
  // per workgroup of ST_BLK queries: its emitted queries (scanned in place) and its rows per verdict
  uint64_t *blk_emit, *blk_cnt;
  uint64_t nblk;
  uint64_t *ctl;  // [0] the emitted queries
};

// drp_digest.hip: the bucket digest of the select's candidates whose ranges lie inside the wire
// (dig_cells: cells, totals), and the count step of the select restricted to the buckets of a set
// (dig_count: bucket_set; sel's scratch and outputs as drp_select.hip's)
struct DigestParams {
  SelectParams sel;
  uint32_t bits;    // 0 .. DRP_DIGEST_MAX_BITS: 2^bits cells, bucket = the identity hash's high bits
  uint32_t chunks;  // dig_cells: chunks of SEL_BLK consecutive rows per workgroup (set by the launcher)
  drp_digest_cell *cells;  // zero before dig_cells
  uint64_t *totals;        // zero before dig_cells; may be null
  const uint64_t *bucket_set;
};
// up to this many bits a workgroup of dig_cells sums into a copy of the cells in LDS (16 KB) and adds
// its non-empty cells to the global ones at its end; above, every row adds to the global cells
constexpr uint32_t DIG_LDS_BITS = 10;
// a dig_cells workgroup takes up to DIG_CHUNKS chunks of SEL_BLK consecutive rows, one row per lane (the
// more rows, the more of them share a cell of its LDS copy), but no more than leave DIG_GRID_MIN
// workgroups: a small batch of long values needs the compute units more than the sharing
constexpr uint32_t DIG_CHUNKS = 4, DIG_GRID_MIN = 128;

// drp_digest.hip: the second level inside the buckets of d.bucket_set (include/drp.h "refined
// digests"). dig_rank leaves rank[w] = the set bits of the set's words before word w, and the set
// bits of all of them (n_set) in d.totals[2]; dig_refine sums d's candidates of the set buckets into
// d.cells[slot(bucket) << sub_bits | sub] (d.totals: three entries, required), dig_count2 keeps those
// whose cell's bit is set in cell_set
struct RefineParams {
  DigestParams d;
  uint32_t sub_bits;     // 1 .. DRP_DIGEST_MAX_SUB_BITS
  uint32_t set_words;    // the words of d.bucket_set: max(1, 2^bits / 64) <= DIG_RANK_BLK
  uint32_t *rank;        // [set_words], scratch
  uint64_t cells_cap;    // dig_refine writes d.cells only if n_set << sub_bits <= cells_cap
  const uint64_t *cell_set;
};
constexpr uint32_t DIG_RANK_BLK = 1024;  // one workgroup, one word of the set per lane
// up to this many second-level cells a dig_refine workgroup sums into a copy in LDS, as dig_cells does
// up to DIG_LDS_BITS bits (DESIGN.md "Refined digests" has the measurement)
constexpr uint32_t DIG_REFINE_LDS_CELLS = 1u << DIG_LDS_BITS;

// drp_order.hip: the segmented order-by-change of encoder rows. A sort workgroup takes ORD_TILE
// (change, row) pairs; a pass's count table holds 256 counts per workgroup and is scanned in
// first-level blocks of ORD_SCAN; passes 0 .. 7 take the key's bytes, pass ORD_SEG_PASS the segment
constexpr uint32_t ORD_TILE = 4096, ORD_SCAN = 1024, ORD_PASSES = 9, ORD_SEG_PASS = 8;
// the control block, written on the device (ord_init, ord_plan)
struct OrdCtl {
  uint64_t n, b0, nwg;  // rows that take part (0: the input is not valid), row_base[0], ceil(n / ORD_TILE)
  uint32_t act[ORD_PASSES], src[ORD_PASSES];  // the pass runs; what it reads (0: the input, 1 / 2: a pair buffer)
  uint32_t final_src, valid;                  // where the finished permutation lies (0: it is the identity)
};
struct OrderParams {
  drp_change_src rows;
  const uint64_t *row_base;  // [nseg + 1]
  uint32_t nseg, flags;
  uint64_t rows_cap;
  RowOut out;               // out.sel_idx: the permuted sel_idx, may be null
  const uint64_t *sel_idx;  // read where out.sel_idx is set
  uint64_t *out_base;       // [nseg + 1]
  uint32_t skip;            // 1: a pass whose digit is the same in every key does not run
  // scratch, placed by the launcher: per sort workgroup the OR and the AND of its keys, two pair
  // buffers of rows_cap entries (keys, rows), the count table, its block sums
  OrdCtl *ctl;
  uint64_t *part_or, *part_and, *key[2];
  uint32_t *idx[2], *hist, *bsum;
  // set by drp_keyorder.hip only (null in drp_order_device): per row, 1 if it takes no part (the
  // segment pass then sorts by 2 * segment + bad, so such rows fall behind their segment's others),
  // and per segment the sorted position, counted from the segment's start, of its first kept row
  const uint8_t *bad;
  const uint64_t *seg_start;
};
// the per-segment limits as a launch argument (UINT64_MAX: none)
struct OrdLimits {
  uint64_t v[DRP_FANOUT_MAX];
};

// drp_keyorder.hip: the segmented order-by-key. The sort is drp_order.hip's digit passes run once per
// field of the tuple (key words, key length, subset presence, subset words, subset length), least
// significant field first; before each run ordk_fetch loads that field of every row, in the order
// reached so far, into the pair buffer's key column.
constexpr uint32_t ORDK_KEY_WORD = 0, ORDK_KEY_LEN = 1, ORDK_SUB_HAS = 2, ORDK_SUB_WORD = 3, ORDK_SUB_LEN = 4;
// written by ordk_prefin; its first 32 bytes are what the host reads to size the launch chain
struct OrdkCtl {
  uint64_t took, left;                 // rows that take part, rows left out
  uint32_t max_key, max_sub, any_sub;  // over the rows that take part: longest key, longest subset, a subset present
  uint32_t shared_words;               // leading 8-byte key words that are whole and equal in all of them
  uint64_t start[DRP_FANOUT_MAX];      // ordk_cut: OrderParams::seg_start
};
// the pages as a launch argument: lo / hi are (offset, length) into the staged bound bytes
struct OrdkPages {
  uint64_t limit[DRP_FANOUT_MAX];
  uint32_t flags[DRP_FANOUT_MAX], lo_off[DRP_FANOUT_MAX], lo_len[DRP_FANOUT_MAX], hi_off[DRP_FANOUT_MAX],
      hi_len[DRP_FANOUT_MAX];
};
struct KeyOrderParams {
  OrderParams o;  // (o.flags: DRP_KEYORDER_KEEP_TIES)
  const uint8_t *heap;
  uint64_t heap_bytes;
  OrdkCtl *kctl;
  uint8_t *bad;           // o.bad, writable (ordk_pre)
  const uint8_t *bounds;  // the staged bound bytes
  uint64_t bounds_bytes;
  uint64_t *totals;       // may be null
};

}  // namespace drp

extern "C" {
void drp_dbg_mark(const char *name, hipStream_t st);  // (drp_api.hip: a named event under DRP_WATCHDOG)
// regions a decode's prologue fills (drp_launch_prologue): byte value, 4-byte multiples
struct ClearSet {
  static constexpr uint32_t CAP = 12;  // (a decode fills up to 9: with records, the density sample and DRP_STATS)
  void *ptr[CAP];
  uint64_t bytes[CAP];
  uint32_t value[CAP];
  uint32_t n;
};
hipError_t drp_launch_prologue(uint32_t B, const uint64_t *stream_off, uint64_t nstreams, uint64_t *tile_prefix,
                               const ClearSet *cs, hipStream_t st);
hipError_t drp_launch_tile_prefix(uint32_t B, const uint64_t *stream_off, uint64_t nstreams,
                                  uint64_t *tile_prefix, hipStream_t st);
hipError_t drp_launch_decode(uint32_t B, const drp::DecodeParams *P, uint32_t grid, hipStream_t st);
uint32_t drp_decode_waves_per_group(void);  // tiles (waves) per workgroup; grid counts groups
uint32_t drp_spec_tile_bytes(void);
uint32_t drp_spec_rec_words(void);  // u32 record words per tile (claims_fast's per-frame records)
uint32_t drp_spec_retry_mask(void);
uint32_t drp_spec_miss_bit(void);
uint32_t drp_spec_cascade_bit(void);
hipError_t drp_launch_claims_walk(const drp::DecodeParams *P, uint64_t nt_max, hipStream_t st);
uint32_t drp_walk_tiles_per_region(uint64_t nt_max, int hop);
hipError_t drp_launch_walk_density(const drp::DecodeParams *P, hipStream_t st);
hipError_t drp_launch_spec_head(const drp::DecodeParams *P, uint64_t nt_max, uint64_t nstreams, hipStream_t st);
// out[0] = payload bytes of the blob rows among rows [0, n) (out zeroed by the caller)
hipError_t drp_launch_blob_bytes(const uint8_t *type, const uint32_t *plen, uint64_t n, uint64_t *out, hipStream_t st);
// ctile: 64 u32 per tile of the range (seg_claims_par; null or too small: the serial seg_claims)
hipError_t drp_launch_seg_repair(const drp::DecodeParams *P, uint64_t s, uint64_t t0, uint64_t tl, uint64_t *scratch,
                                 uint32_t *ctile, uint64_t ctile_cap, hipStream_t st);
hipError_t drp_launch_spec_verify(const drp::DecodeParams *P, uint64_t nt_max, hipStream_t st);
hipError_t drp_launch_spec_verify_list(const drp::DecodeParams *P, uint64_t n, hipStream_t st);
hipError_t drp_launch_spec_tail(const drp::DecodeParams *P, uint64_t nt_max, uint64_t nstreams, uint64_t *scan_tmp,
                                hipStream_t st);
// the tail's scan: tile_count -> tile_base (capacity check) and tile_nch -> tile_nch_base in one
// pass, which also zeroes vlist_n and writes emit_recs' chunk_tile marks; tmp: 2 block-sum arrays
hipError_t drp_launch_tile_scan2(const drp::DecodeParams *P, uint64_t nstreams, uint64_t nt_max, uint64_t *tmp,
                                 hipStream_t st);
// exclusive scan of a per-tile u64 array over all tiles; flags capacity overflow of the total
hipError_t drp_launch_tile_scan(const uint64_t *in, const uint64_t *tile_prefix, uint64_t nstreams, uint64_t nt_max,
                                uint64_t *tmp, uint64_t *out, uint64_t cap, uint32_t *overflow, hipStream_t st);
// per-stream change / blob counts from the per-tile counts and their scans
hipError_t drp_launch_stream_counts(const uint64_t *tile_prefix, uint64_t nstreams, const uint64_t *count,
                                    const uint64_t *base, const uint64_t *nch, const uint64_t *nch_base,
                                    uint64_t *scount, hipStream_t st, uint32_t *total = nullptr);
hipError_t drp_launch_finalize(const uint8_t *bytes, const uint64_t *stream_off, uint64_t nstreams,
                               const uint64_t *tile_prefix, const uint64_t *tile_exit,
                               const uint64_t *tile_base, const uint64_t *tile_count,
                               const uint64_t *payload_err, const uint64_t *scount,
                               const uint8_t *type, const uint8_t *flags, uint64_t cap,
                               drp_stream_result *res, const uint32_t *abort_flag,
                               uint32_t abort_mask, hipStream_t st);
hipError_t drp_launch_encode(const drp::EncodeParams *P, hipStream_t st);
uint64_t drp_encode_out_blocks(uint64_t cap);
// key hash + key flags for every change frame written (no-op when co->key_hash is NULL)
hipError_t drp_launch_key_post(const uint8_t *bytes, const uint64_t *tile_prefix, uint64_t nstreams,
                               const uint64_t *tile_base, const uint64_t *tile_count, uint64_t cap,
                               const drp_frames *fr, const drp_changes *co, int flags_only, const uint32_t *abort_flag,
                               uint32_t abort_mask, hipStream_t st);
uint64_t drp_select_scratch_bytes(uint64_t n);  // device scratch drp_launch_select needs for n rows
uint32_t drp_select_known_flags(void);
hipError_t drp_launch_select(const drp::SelectParams *P, const drp::SelectBytes *fb, void *scratch, hipStream_t st);
// its pieces, for drp_latest.hip: the scratch pointers and the filter's bytes (n > 0), and the scan
// and scatter over the ballot words and workgroup counts already in P's scratch
hipError_t drp_select_place(drp::SelectParams *P, const drp::SelectBytes *fb, void *scratch, hipStream_t st);
hipError_t drp_launch_select_compact(const drp::SelectParams *P, hipStream_t st);
// drp_latest.hip. Scratch: the select's (drp_select_scratch_bytes(n)), then slot[n], then the table.
uint64_t drp_latest_scratch_bytes(uint64_t n);
hipError_t drp_launch_latest(const drp::SelectParams *P, const drp::SelectBytes *fb, uint64_t hash_mask,
                             void *scratch, hipStream_t st);
// drp_fanout.hip. Scratch layout (drp_fanout_place sets P's scratch pointers from it): the filter
// table, the byte strings, the ballot planes, the counts, the block sums, the grand total.
uint64_t drp_fanout_scratch_bytes(uint64_t n, uint32_t nfilters);
void drp_fanout_place(drp::FanParams *P, void *scratch);
// count + scan: P->row_base[0 .. nfilters] and *P->gtotal (rows + blob rows) are written
hipError_t drp_launch_fanout_count(const drp::FanParams *P, hipStream_t st);
// its two halves: the ballot planes with their workgroup counts, and the scan of whatever counts
// P's scratch holds (drp_launch_fanout_latest rewrites planes and counts in between)
hipError_t drp_launch_fanout_ballot(const drp::FanParams *P, hipStream_t st);
hipError_t drp_launch_fanout_scan(const drp::FanParams *P, hipStream_t st);
// drp_latest.hip, between those two: every filter's plane and counts cut down to the plane's latest
// row per key, `pass` filters (1 .. nfilters) per reduction pass. Scratch: the fan-out's
// (drp_fanout_scratch_bytes, placed in P already), then group[n], the table's rep words, the claim
// ballots and their scan, the pass state.
uint64_t drp_fanout_latest_scratch_bytes(uint64_t n, uint32_t nfilters, uint32_t pass);
hipError_t drp_launch_fanout_latest(const drp::FanParams *P, uint64_t hash_mask, uint32_t pass, void *scratch,
                                    hipStream_t st);
// drp_select.hip's scan on its own: cnt[0, nblk) scanned in place (exclusive), *total = their sum
hipError_t drp_launch_count_scan(uint64_t *cnt, uint64_t nblk, uint64_t *total, hipStream_t st);
// drp_store.hip. The table's slots for max_keys (0: out of range); an empty store; steps 2 to 6 of a
// merge over the winners in M (its state is placed in `scratch`, drp_store_merge_scratch_bytes(n)
// bytes), then, with a report R (null: none), the rep_* steps; a compact into arena2 (scratch:
// drp_store_compact_scratch_bytes(max_keys)).
uint64_t drp_store_nslots(uint64_t max_keys);
hipError_t drp_launch_store_init(const drp::StoreDev *S, hipStream_t st);
uint64_t drp_store_merge_scratch_bytes(uint64_t n);
hipError_t drp_launch_store_merge(const drp::StoreMerge *M, const drp::StoreReport *R, void *scratch, hipStream_t st);
uint64_t drp_store_blocks(uint64_t n);  // the workgroups of ST_BLK winners a merge of n rows runs (>= 1)
// the load (include/drp.h "store lifecycle") of the rows in M, a select's and taken to be new: the
// merge's steps with stl_plan in st_lookup's place (the same state in `scratch`), then, with `clash`
// (device, null: none), the self-check of the rows it added. The rehash: the table rebuilt from the
// rows in use under S->hash_mask, with `report` (device, two words, null: none) the invalid rows and
// the self-check of all of them; no scratch
hipError_t drp_launch_store_load(const drp::StoreMerge *M, uint64_t *clash, void *scratch, hipStream_t st);
hipError_t drp_launch_store_rehash(const drp::StoreDev *S, uint64_t *report, hipStream_t st);
// the lookup Q (its state is placed in `scratch`, drp_store_lookup_scratch_bytes(n) bytes; fb: the
// filter's byte strings, as drp_launch_select takes them): nothing of the store is written
uint64_t drp_store_lookup_scratch_bytes(uint64_t n);
hipError_t drp_launch_store_lookup(const drp::StoreLookup *Q, const drp::SelectBytes *fb, void *scratch,
                                   hipStream_t st);
uint64_t drp_store_compact_scratch_bytes(uint64_t max_keys);
hipError_t drp_launch_store_compact(const drp::StoreDev *S, uint8_t *arena2, uint64_t arena2_bytes, void *scratch,
                                    hipStream_t st);
// drp_digest.hip. The cells and totals of D (both cleared first); bucket_set and *n_diff from two cell
// arrays of 2^bits; the select over D's candidates in the buckets of D->bucket_set (scratch:
// drp_select_scratch_bytes(n), as drp_launch_select; drp_launch_digest takes its first
// 2 * DRP_SEL_MAX_BYTES bytes for the filter's byte strings)
hipError_t drp_launch_digest(const drp::DigestParams *D, const drp::SelectBytes *fb, void *scratch, hipStream_t st);
hipError_t drp_launch_digest_diff(const drp_digest_cell *a, const drp_digest_cell *b, uint32_t bits,
                                  uint64_t *bucket_set, uint64_t *n_diff, hipStream_t st);
hipError_t drp_launch_select_buckets(const drp::DigestParams *D, const drp::SelectBytes *fb, void *scratch,
                                     hipStream_t st);
// The second level. drp_launch_digest_diff for any cell count (0: the one word and *n_diff are 0);
// the refine (scratch: 2 * DRP_SEL_MAX_BYTES bytes, then R->rank, placed by the caller); the select of
// the set cells' rows (scratch: drp_select_scratch_bytes(n), R->rank behind it)
hipError_t drp_launch_digest_diff_cells(const drp_digest_cell *a, const drp_digest_cell *b, uint32_t ncell,
                                        uint64_t *cell_set, uint64_t *n_diff, hipStream_t st);
hipError_t drp_launch_digest_refine(const drp::RefineParams *R, const drp::SelectBytes *fb, void *scratch,
                                    hipStream_t st);
hipError_t drp_launch_select_refined(const drp::RefineParams *R, const drp::SelectBytes *fb, void *scratch,
                                     hipStream_t st);
// drp_order.hip. Scratch for rows_cap entries: 24 bytes per entry (two buffers of 8-byte keys and
// 4-byte rows) and 1 KiB of counts, 16 bytes of key bits and 1 byte of block sums per ORD_TILE
// entries. out_max: an upper bound of the rows all outputs hold together (the limits' sum, saturated;
// with DRP_ORDER_KEEP_TIES an output may pass its limit: ~0).
uint64_t drp_order_scratch_bytes(uint64_t rows_cap);
hipError_t drp_launch_order(const drp::OrderParams *P, const drp::OrdLimits *lim, uint64_t out_max, void *scratch,
                            hipStream_t st);
// drp_keyorder.hip. Scratch: drp_order_scratch_bytes(rows_cap), then one byte per entry of rows_cap,
// the OrdkCtl and bounds_bytes of staged bounds. bounds_host (bounds_bytes, may be null when 0) is
// copied to the device and may be freed when the call returns. Waits for the stream once (the longest
// key and subset size the launch chain).
uint64_t drp_keyorder_scratch_bytes(uint64_t rows_cap, uint64_t bounds_bytes);
hipError_t drp_launch_keyorder(const drp::KeyOrderParams *K, const drp::OrdkPages *pages, const uint8_t *bounds_host,
                               uint64_t out_max, void *scratch, hipStream_t st);
hipError_t drp_launch_fanout_scatter(const drp::FanParams *P, hipStream_t st);
hipError_t drp_launch_fanout_splice(const drp::FanParams *P, hipStream_t st);
// out_off[f] = frame_off[row_base[f]] (f <= nfilters); blob_pos[f * nb + j] = frame_off[row_base[f] +
// rank[f * nb + j]] - out_off[f]
hipError_t drp_launch_fanout_gather(const uint64_t *frame_off, const uint64_t *row_base, uint32_t nfilters,
                                    const uint64_t *rank, uint64_t nb, uint64_t *out_off, uint64_t *blob_pos,
                                    hipStream_t st);
hipError_t drp_launch_index_scan(const drp_stream_stats *stats, uint64_t count, uint64_t *base,
                                 hipStream_t st);
hipError_t drp_launch_stats_from_results(const drp_stream_result *res, const uint64_t *stream_off,
                                         uint64_t nstreams, drp_stream_stats *stats, hipStream_t st);
}
