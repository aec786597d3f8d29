"""ctypes binding of libdrp (include/drp.h) for the Python test suite and bench.py.

The product host layer is the Node module in this package (index.js / decode.js /
encode.js over the N-API addon); this module exposes the same C ABI to Python so the
parity tests and the benchmark call exactly the code the addon calls. It loads the
in-tree lib/libdrp.so and raises if it is missing: there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("DRP_LIB") or os.path.join(PKG, "lib", "libdrp.so")
if not os.path.isabs(LIB_PATH):  # (an A/B build named relative to the repo root: exp/<name>/libdrp.so)
    LIB_PATH = os.path.join(os.path.dirname(PKG), LIB_PATH)

DRP_OK, DRP_E_INVAL, DRP_E_HIP, DRP_E_NOMEM, DRP_E_CAPACITY, DRP_E_NODEV = 0, -1, -2, -3, -4, -5
TYPE_CHANGE, TYPE_BLOB, FRAME_CONT, FRAME_PARTIAL = 1, 2, 0x40, 0x80
F_SUBSET, F_VALUE, F_BAD, F_MISSING, F_KEY_ASCII, F_KEY_UTF8 = 1, 2, 4, 8, 0x10, 0x20
ERR_NONE, ERR_TYPE, ERR_LEN, ERR_VARINT, ERR_CHANGE, ERR_REQUIRED = 0, 1, 2, 3, 4, 5
TAIL_NONE, TAIL_HEADER, TAIL_CHANGE, TAIL_BLOB = 0, 1, 2, 3
KEY_POST_OFF, KEY_POST_HASH, KEY_POST_FLAGS = 0, 1, 2
BLOB_SKIP_OFF, BLOB_SKIP_AUTO, BLOB_SKIP_ALWAYS = 0, 1, 2
DRP_E_COMM = -7
SEL_CHANGE_RANGE, SEL_SUBSET_EQ, SEL_SUBSET_NONE, SEL_KEY_PREFIX = 1, 2, 4, 8
SEL_MAX_BYTES = 256
FANOUT_MAX = 64
DIGEST_MAX_BITS = 16
DIGEST_MAX_SUB_BITS = 8
ORDER_KEEP_TIES = 1
KEYORDER_KEEP_TIES, KEYORDER_MAX_BYTES = 1, 4096
KEYPAGE_FROM, KEYPAGE_AFTER, KEYPAGE_UNTIL = 1, 2, 4
MERGE_NONE, MERGE_INSERTED, MERGE_REPLACED, MERGE_UNCHANGED, MERGE_STALE, MERGE_SKIPPED = 0, 1, 2, 3, 4, 5
REPORT_KEEP_BLOBS = 1
LOOKUP_NONE, LOOKUP_ABSENT, LOOKUP_BEHIND, LOOKUP_LEVEL, LOOKUP_AHEAD = 0, 1, 2, 3, 4
LOOKUP_FOUND = (1 << LOOKUP_BEHIND) | (1 << LOOKUP_LEVEL) | (1 << LOOKUP_AHEAD)  # the emit_mask of a multi-get
LOOKUP_REPLY_LACK = 0x100
ORDER_TILE, ORDER_SCAN = 4096, 1024  # csrc/drp_kernels.h ORD_TILE, ORD_SCAN: pairs per sort workgroup, counts per scan block
DIGEST_LDS_BITS = 10  # csrc/drp_kernels.h DIG_LDS_BITS: up to here dig_cells sums in LDS, above in global memory
COMM_ID_BYTES = 128

P = C.c_void_p
U64, U32 = C.c_uint64, C.c_uint32


class Frames(C.Structure):
    _fields_ = [("payload_off", P), ("payload_len", P), ("type", P)]


class Changes(C.Structure):
    _fields_ = [(k, P) for k in ["key_off", "key_len", "subset_off", "subset_len", "value_off",
                                 "value_len", "change", "from_", "to", "flags", "key_hash"]]


class ChangeSrc(C.Structure):
    _fields_ = [(k, P) for k in ["key_off", "key_len", "subset_off", "subset_len", "value_off",
                                 "value_len", "change", "from_", "to", "flags"]]


class Carry(C.Structure):
    _fields_ = [("blob_remaining", U64), ("consumed", U64), ("tail_kind", U32), ("reserved", U32),
                ("frame_bytes", U64)]


class StreamResult(C.Structure):
    _fields_ = [("frame_begin", U64), ("frames", U64), ("changes", U64), ("blobs", U64),
                ("consumed", U64), ("blob_remaining", U64), ("err_frame", U64), ("err_code", U32),
                ("err_detail", U32), ("tail_kind", U32), ("reserved", U32), ("tail_frame_bytes", U64)]


class StreamStats(C.Structure):
    _fields_ = [("frames", U64), ("changes", U64), ("blobs", U64), ("wire_bytes", U64)]


class Chunk(C.Structure):
    _fields_ = [("bytes", P), ("n", U64)]


class Filter(C.Structure):
    """drp_filter; make one with make_filter (it keeps the byte strings alive)."""
    _fields_ = [("flags", U32), ("subset_len", U32), ("key_prefix_len", U32), ("reserved", U32),
                ("change_min", U64), ("change_max", U64), ("subset", P), ("key_prefix", P)]


def make_filter(change_range=None, subset=None, subset_none=False, key_prefix=None, flags=None):
    """A drp_filter: change_range=(min, max) inclusive, subset=bytes (present and equal),
    subset_none=True (absent), key_prefix=bytes; the conditions AND together. flags overrides
    the flag word (tests of the error returns)."""
    f = Filter()
    fl = 0
    if change_range is not None:
        fl |= SEL_CHANGE_RANGE
        f.change_min, f.change_max = int(change_range[0]), int(change_range[1])
    f._keep = []
    if subset is not None:
        fl |= SEL_SUBSET_EQ
        b = C.create_string_buffer(bytes(subset), max(1, len(subset)))
        f._keep.append(b)
        f.subset, f.subset_len = C.cast(b, P), len(subset)
    if subset_none:
        fl |= SEL_SUBSET_NONE
    if key_prefix is not None:
        fl |= SEL_KEY_PREFIX
        b = C.create_string_buffer(bytes(key_prefix), max(1, len(key_prefix)))
        f._keep.append(b)
        f.key_prefix, f.key_prefix_len = C.cast(b, P), len(key_prefix)
    f.flags = fl if flags is None else flags
    return f


class KeyPage(C.Structure):
    """drp_key_page; make one with make_key_page (it keeps the bound bytes alive)."""
    _fields_ = [("flags", U32), ("lo_len", U32), ("hi_len", U32), ("reserved", U32), ("lo", P), ("hi", P),
                ("limit", U64)]


def make_key_page(from_=None, after=None, until=None, limit=None, flags=None):
    """A drp_key_page: from_=bytes keeps key >= from_, after=bytes keeps key > after (a resume
    cursor; not together with from_), until=bytes keeps key < until, limit=rows (None: no limit). An
    empty bound is a bound. flags overrides the flag word (tests of the error returns)."""
    g = KeyPage()
    g._keep = []
    fl = 0

    def put(b):
        buf = C.create_string_buffer(bytes(b), max(1, len(b)))
        g._keep.append(buf)
        return C.cast(buf, P), len(b)

    if from_ is not None:
        fl |= KEYPAGE_FROM
        g.lo, g.lo_len = put(from_)
    if after is not None:
        fl |= KEYPAGE_AFTER
        g.lo, g.lo_len = put(after)
    if until is not None:
        fl |= KEYPAGE_UNTIL
        g.hi, g.hi_len = put(until)
    g.limit = 0xFFFFFFFFFFFFFFFF if limit is None else int(limit)
    g.flags = fl if flags is None else flags
    return g


def key_page_array(pages):
    """A C array of drp_key_page from make_key_page results (None: the page that keeps everything).
    Keeps the pages, and with them their bound bytes, alive."""
    arr = (KeyPage * max(1, len(pages)))()
    arr._keep = list(pages)
    for k, g in enumerate(pages):
        if g is not None:
            C.memmove(C.byref(arr, k * C.sizeof(KeyPage)), C.byref(g), C.sizeof(KeyPage))
        else:
            arr[k].limit = 0xFFFFFFFFFFFFFFFF
    return arr


class Splice(C.Structure):
    """drp_splice: the optional splice outputs of drp_fanout_device (device pointers)."""
    _fields_ = [("blob_row", P), ("blob_rank", P), ("n_blobs", P), ("blob_cap", U64)]


def filter_array(filters):
    """A C array of drp_filter from make_filter results (None: the filter that keeps every
    well-formed Change). Keeps the filters, and with them their byte strings, alive."""
    arr = (Filter * max(1, len(filters)))()
    arr._keep = list(filters)
    for k, f in enumerate(filters):
        if f is not None:
            C.memmove(C.byref(arr, k * C.sizeof(Filter)), C.byref(f), C.sizeof(Filter))
    return arr


class StoreInfo(C.Structure):
    """drp_store_info: the store's record (device memory; store_query copies it out)."""
    _fields_ = [(k, U64) for k in ["rows", "arena_used", "arena_dead", "merges", "winners", "inserted", "replaced",
                                   "unchanged", "stale", "skipped", "refused", "need_rows", "need_bytes",
                                   "reserved"]]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class StoreDesc(C.Structure):
    """drp_store: a host struct of device pointers; the Store helper below builds one."""
    _fields_ = [("arena", P), ("arena_bytes", U64), ("frames", Frames), ("cols", Changes), ("max_keys", U64),
                ("table", P), ("info", P), ("reserved", U64)]


class MergeReport(C.Structure):
    """drp_merge_report: a host struct of device pointers (reply_rows: a host pointer to a ChangeSrc)."""
    _fields_ = [("flags", U32), ("reserved", U32), ("outcome", P), ("news_type", P), ("reply_rows", C.POINTER(ChangeSrc)),
                ("reply_idx", P), ("n_reply", P), ("reply_cap", U64), ("reserved2", U64)]


class Lookup(C.Structure):
    """drp_lookup: a host struct of device pointers (out_rows: a host pointer to a ChangeSrc)."""
    _fields_ = [("flags", U32), ("emit_mask", U32), ("verdict", P), ("hit_row", P), ("counts", P), ("lack_type", P),
                ("out_rows", C.POINTER(ChangeSrc)), ("out_query", P), ("n_out", P), ("rows_cap", U64), ("reserved", U64),
                ("reserved2", U64)]


def lookup_bit(code):
    """DRP_LOOKUP_BIT: the emit_mask bit of a verdict code."""
    return 1 << code


class DigestCell(C.Structure):
    """drp_digest_cell: the rows of one bucket and the sum of their fingerprints (mod 2^64)."""
    _fields_ = [("count", U64), ("sum", U64)]


class Timing(C.Structure):
    _fields_ = [("decode_ms", C.c_float), ("finalize_ms", C.c_float), ("total_ms", C.c_float),
                ("strict_reruns", U32), ("spec_repairs", U32), ("exact_retries", U32), ("verify_relisted", U32),
                ("seg_repairs", U32), ("reserved", U32), ("h2d_ms", C.c_float), ("d2h_ms", C.c_float),
                ("h2d_bytes", U64), ("h2d_skipped", U64), ("host_copied", U64)]


COLS32 = ["key_off", "key_len", "subset_off", "subset_len", "value_off", "value_len"]
COLS64 = ["change", "from", "to"]
SRC_COLS = COLS32 + COLS64 + ["flags"]  # the fields of drp_change_src, in order

# ---- the bound ABI: name -> (restype, argtypes), one entry per declaration of include/drp.h --------
INT = C.c_int
PP, PU64, PU32 = C.POINTER(P), C.POINTER(U64), C.POINTER(U32)
PFrames, PChanges, PSrc, PFilter = C.POINTER(Frames), C.POINTER(Changes), C.POINTER(ChangeSrc), C.POINTER(Filter)
PCarry, PStore, PInfo = C.POINTER(Carry), C.POINTER(StoreDesc), C.POINTER(StoreInfo)
# the argument runs that recur
_BATCH = [P, P, U64, PFrames, PChanges, U64, PFilter]  # ctx, bytes, nbytes, frames, cols, n, filter(s)
_STORE = [P, PStore] + _BATCH[1:]                      # ctx, store, then that batch
_STAGE_OUT = [PCarry, PU64, PU64, PU32, PU32]          # carry, n_frames, err_frame, err_code, err_detail
_SELECT_OUT = [PSrc, P, P]                             # out_rows, sel_idx, n_selected
_FANOUT_OUT = [U32, PSrc, U64, P, P]                   # nfilters, out_rows, rows_cap, sel_idx, row_base
_RELAY_STAGED = [P, PFilter, P, U64, PU64, PU64]       # ctx, filter, out, cap, written, n_selected
_FANOUT_STAGED = [P, PFilter, U32, P, U64, P, P]       # ctx, filters, nfilters, out, cap, out_off, n_selected
_FANOUT_BLOBS = [P, P, U64, P]                         # blob_row, blob_pos, blob_cap, n_blobs
_MERGE_STAGED = [P, PStore, PFilter, PInfo]            # ctx, store, filter, info_host
_ORDER_OUT = [PSrc, P, P, P]                           # out_rows, sel_idx, out_sel_idx, out_base
_GATHER_MULTI = [PP, PP, INT, PP, U64]                 # ctxs, comms, ngpu, local, per_gpu

SIGNATURES = {
    "drp_abi_version": (INT, []),
    "drp_open": (INT, [INT, PP]),
    "drp_close": (None, [P]),
    "drp_stream": (P, [P]),
    "drp_synchronize": (INT, [P]),
    "drp_last_timing": (INT, [P, C.POINTER(Timing)]),
    "drp_set_tile": (INT, [P, U32]),
    "drp_set_strict": (INT, [P, INT]),
    "drp_set_exact": (INT, [P, INT]),
    "drp_set_key_post": (INT, [P, INT]),
    "drp_set_blob_skip": (INT, [P, INT]),
    "drp_decode_scratch_bytes": (U64, [P, U64, U64]),
    "drp_decode_device": (INT, [P, P, U64, P, P, U64, PFrames, PChanges, U64, P]),
    "drp_decode_batch": (INT, [P, P, U64, PCarry, PFrames, PChanges, U64] + _STAGE_OUT[1:]),
    "drp_decode_stage": (INT, [P, P, U64] + _STAGE_OUT),
    "drp_decode_stage_v": (INT, [P, C.POINTER(Chunk), U64] + _STAGE_OUT),
    "drp_decode_fetch": (INT, [P, PFrames, PChanges, U64, U64]),
    "drp_decode_fetch_block": (INT, [P, P, U64, PU64, U64, U64]),
    "drp_decode_fetch_block_ex": (INT, [P, P, U64, PU64, U64, U64, U32]),
    "drp_decode_fetch_keys": (INT, [P, U64, U64, P, P, U64, PU64]),
    "drp_encode_size": (INT, [P, PSrc, U64, PU64]),
    "drp_encode_device": (INT, [P, PSrc, P, U64, U64, P, P, U64]),
    "drp_encode_batch": (INT, [P, PSrc, P, U64, U64, P, U64, PU64]),
    "drp_select_device": (INT, _BATCH + _SELECT_OUT),
    "drp_relay_staged": (INT, _RELAY_STAGED),
    "drp_index_scan": (INT, [P, P, U64, P]),
    "drp_stream_stats_from_results": (INT, [P, P, P, U64, P]),
    "drp_device": (INT, [P]),
    "drp_fanout_device": (INT, _BATCH + _FANOUT_OUT + [C.POINTER(Splice)]),
    "drp_fanout_staged": (INT, _FANOUT_STAGED + _FANOUT_BLOBS),
    "drp_latest_device": (INT, _BATCH + _SELECT_OUT),
    "drp_latest_staged": (INT, _RELAY_STAGED),
    "drp_set_latest_hash_mask": (INT, [P, U64]),
    "drp_fanout_latest_device": (INT, _BATCH + _FANOUT_OUT),
    "drp_fanout_latest_staged": (INT, _FANOUT_STAGED),
    "drp_set_fanout_latest_pass": (INT, [P, U32]),
    "drp_store_table_bytes": (U64, [U64]),
    "drp_store_init": (INT, [P, PStore]),
    "drp_store_merge_device": (INT, _STORE),
    "drp_store_merge_staged": (INT, _MERGE_STAGED),
    "drp_store_compact": (INT, [P, PStore, P, U64]),
    "drp_store_query": (INT, [P, PStore, PInfo]),
    "drp_order_device": (INT, [P, PSrc, P, U32, U64, P, U32] + _ORDER_OUT),
    "drp_order_keys_device": (INT, [P, P, U64, PSrc, P, U32, U64, C.POINTER(KeyPage), U32] + _ORDER_OUT + [P]),
    "drp_store_merge_report_device": (INT, _STORE + [C.POINTER(MergeReport)]),
    "drp_store_merge_news_staged": (INT, _MERGE_STAGED),
    "drp_fanout_news_staged": (INT, _FANOUT_STAGED + _FANOUT_BLOBS),
    "drp_store_lookup_device": (INT, _STORE + [C.POINTER(Lookup)]),
    "drp_store_lookup_staged": (INT, [P, PStore, PFilter, U32, P, U64, PU64, PU64, PU64]),
    "drp_store_load_device": (INT, _STORE + [P]),
    "drp_store_rehash_device": (INT, [P, PStore, P]),
    "drp_digest_device": (INT, _BATCH + [U32, P, P]),
    "drp_digest_diff_device": (INT, [P, P, P, U32, P, P]),
    "drp_select_buckets_device": (INT, _BATCH + [U32, P] + _SELECT_OUT),
    "drp_digest_refine_device": (INT, _BATCH + [U32, P, U32, P, U64, P]),
    "drp_digest_diff_cells_device": (INT, [P, P, P, U64, P, P]),
    "drp_select_refined_device": (INT, _BATCH + [U32, P, U32, P] + _SELECT_OUT),
    "drp_comm_id": (INT, [P]),
    "drp_comm_init_rank": (INT, [P, P, INT, INT, PP]),
    "drp_comm_init_all": (INT, [PP, INT, PP]),
    "drp_comm_destroy": (None, [P]),
    "drp_index_allgather": (INT, [P, P, P, U64, P, P]),
    "drp_index_allgather_multi": (INT, _GATHER_MULTI + [PP, PP]),
    "drp_index_allgather_host": (INT, _GATHER_MULTI + [P, P]),
    "drp_device_count": (INT, [C.POINTER(INT)]),
    "drp_host_alloc": (INT, [U64, PP]),
    "drp_host_free": (None, [P]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    """Load lib/libdrp.so (raises OSError if it was not built: no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"libdrp not built: {LIB_PATH} missing (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


class DrpError(RuntimeError):
    def __init__(self, fn, rc):
        super().__init__(f"{fn} failed with {rc}")
        self.rc = rc


def _chk(fn, rc, **attrs):
    """Raise DrpError(fn, rc) unless rc is DRP_OK; attrs become attributes of the error (.written,
    .n_selected, .info: what a call that ran out of capacity still reports)."""
    if rc != DRP_OK:
        e = DrpError(fn, rc)
        e.__dict__.update(attrs)
        raise e


# ---- marshalling: numpy arrays, torch tensors and column dicts as the ABI's pointers and structs ----
def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _tp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ref(s):
    return C.byref(s) if s is not None else None


def alloc_host_outputs(cap, key_hash=False):
    o = {"payload_off": np.zeros(cap, np.uint64), "payload_len": np.zeros(cap, np.uint32),
         "type": np.zeros(cap, np.uint8), "flags": np.zeros(cap, np.uint8)}
    if key_hash:
        o["key_hash"] = np.zeros(cap, np.uint64)
    for k in COLS32:
        o[k] = np.zeros(cap, np.uint32)
    for k in COLS64:
        o[k] = np.zeros(cap, np.uint64)
    return o


def _structs(o, ptr):
    """drp_frames and drp_changes over a dict of columns (numpy with _p, torch with _tp); payload_len
    and key_hash may be missing."""
    opt = lambda k: ptr(o[k]) if o.get(k) is not None else None
    fr = Frames(ptr(o["payload_off"]), opt("payload_len"), ptr(o["type"]))
    co = Changes(*[ptr(o[k]) for k in COLS32 + COLS64], ptr(o["flags"]), opt("key_hash"))
    return fr, co


def _batch(wire_t, cols, n):
    """The arguments bytes, nbytes, frames, cols, n of a *_device call over a decoded batch."""
    fr, co = _structs(cols, _tp)
    return _tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n


def _src(rows, ptr=_tp):
    """drp_change_src over a dict of row columns (None: None); a missing column is passed as NULL,
    which the library answers with DRP_E_INVAL."""
    return ChangeSrc(*[ptr(rows.get(k)) for k in SRC_COLS]) if rows is not None else None


class Ctx:
    """One libdrp context (device + HIP stream + scratch)."""

    def __init__(self, device=0, tile=0):
        self.L = lib()
        h = P()
        _chk("drp_open", self.L.drp_open(device, C.byref(h)))
        self.h = h
        if tile:
            _chk("drp_set_tile", self.L.drp_set_tile(self.h, tile))

    def close(self):
        if self.h:
            self.L.drp_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self):
        return self.L.drp_stream(self.h)

    # libdrp launches on its own non-blocking HIP stream: work torch queued on its current
    # stream (allocations, fills, copies producing our inputs) must be ordered before a
    # libdrp call, and torch must not read libdrp outputs before libdrp's stream is done.
    def _ext(self, dev):
        import torch
        ext = getattr(self, "_ext_stream", None)
        if ext is None or ext.device != dev:
            ext = torch.cuda.ExternalStream(self.stream, device=dev)
            self._ext_stream = ext
        return ext

    def order_after_torch(self, t):
        """libdrp's stream waits for the work queued so far on torch's current stream (nothing
        to do when torch's current stream is libdrp's own, e.g. under torch.cuda.stream(...))."""
        import torch
        ext, cur = self._ext(t.device), torch.cuda.current_stream(t.device)
        if cur.cuda_stream != ext.cuda_stream:
            ext.wait_stream(cur)

    def order_torch_after(self, t):
        """torch's current stream waits for the work queued so far on libdrp's stream."""
        import torch
        ext, cur = self._ext(t.device), torch.cuda.current_stream(t.device)
        if cur.cuda_stream != ext.cuda_stream:
            cur.wait_stream(ext)

    def set_strict(self, on):
        _chk("drp_set_strict", self.L.drp_set_strict(self.h, 1 if on else 0))

    def set_exact(self, on):
        """Force the exact decode kernel (else: speculate-and-verify with exact fallback)."""
        _chk("drp_set_exact", self.L.drp_set_exact(self.h, 1 if on else 0))

    def set_blob_skip(self, mode):
        """Host batches: BLOB_SKIP_AUTO (default), _ALWAYS (every batch in blob-skipping
        pieces) or _OFF (every batch staged whole); results are identical."""
        _chk("drp_set_blob_skip", self.L.drp_set_blob_skip(self.h, mode))

    def set_tile(self, tile):
        _chk("drp_set_tile", self.L.drp_set_tile(self.h, tile))

    def timing(self):
        t = Timing()
        _chk("drp_last_timing", self.L.drp_last_timing(self.h, C.byref(t)))
        return t

    # ---- host-buffer batch decode (the N-API addon's path) -----------------------------
    def decode_batch(self, wire, blob_remaining=0, cap=None, key_hash=False, outs=None):
        """drp_decode_batch into host columns; key_hash=True also asks for the key hash
        column and the DRP_F_KEY_ASCII / DRP_F_KEY_UTF8 flags. outs: host columns to reuse
        (alloc_host_outputs(cap))."""
        w = np.frombuffer(bytes(wire), np.uint8) if not isinstance(wire, np.ndarray) else wire
        n = int(w.size)
        if outs is not None:
            cap = int(outs["payload_off"].size)
        elif cap is None:
            cap = n // 2 + 2
        o = outs if outs is not None else alloc_host_outputs(cap, key_hash)
        fr, co = _structs(o, _p)
        carry = Carry(blob_remaining, 0, 0, 0, 0)
        nf, ef, ec, ed = U64(), U64(), U32(), U32()
        buf = w if n else np.zeros(16, np.uint8)
        rc = self.L.drp_decode_batch(self.h, _p(buf), n, C.byref(carry), C.byref(fr), C.byref(co),
                                     cap, C.byref(nf), C.byref(ef), C.byref(ec), C.byref(ed))
        _chk("drp_decode_batch", rc)
        nframes = int(nf.value)
        keep = nframes + (1 if ec.value in (ERR_CHANGE, ERR_REQUIRED) else 0)
        res = {k: v[:keep] for k, v in o.items()}
        res.update(nframes=nframes, err_frame=int(ef.value), err_code=int(ec.value),
                   err_detail=int(ed.value), consumed=int(carry.consumed),
                   tail=int(carry.tail_kind), blob_remaining=int(carry.blob_remaining),
                   frame_bytes=int(carry.frame_bytes))
        return res

    def decode_staged(self, wire, blob_remaining=0, pieces=1, key_hash=False, block=False, f64=False, keys=False):
        """drp_decode_stage, then drp_decode_fetch of the rows in `pieces` consecutive
        fetches into host columns sized from the frame count (the N-API addon's path). `wire`
        as a list of byte strings: the batch is those chunks end to end (drp_decode_stage_v).
        block=True: one drp_decode_fetch_block of every row into one host block instead (the
        columns at 64-byte aligned offsets, as the addon lays them out); f64=True: with
        drp_decode_fetch_block_ex(DRP_FETCH_F64), payload_off / change / from / to as float64.
        keys=True: the key flags too, and drp_decode_fetch_keys' "kp" (u32 per row) and "key_text"
        (bytes; None when the batch was staged in pieces: DRP_E_INVAL)."""
        carry = Carry(blob_remaining, 0, 0, 0, 0)
        nf, ef, ec, ed = U64(), U64(), U32(), U32()
        kpost = KEY_POST_HASH if key_hash else (KEY_POST_FLAGS if keys else KEY_POST_OFF)
        _chk("drp_set_key_post", self.L.drp_set_key_post(self.h, kpost))
        if isinstance(wire, (list, tuple)):
            arrs = [np.frombuffer(bytes(c), np.uint8) if len(c) else np.zeros(1, np.uint8) for c in wire]
            ch = (Chunk * max(1, len(arrs)))(*[Chunk(_p(a), len(c)) for a, c in zip(arrs, wire)])
            _chk("drp_decode_stage_v", self.L.drp_decode_stage_v(self.h, ch, len(arrs), C.byref(carry), C.byref(nf),
                                                                 C.byref(ef), C.byref(ec), C.byref(ed)))
        else:
            w = np.frombuffer(bytes(wire), np.uint8) if not isinstance(wire, np.ndarray) else wire
            n = int(w.size)
            buf = w if n else np.zeros(16, np.uint8)
            _chk("drp_decode_stage", self.L.drp_decode_stage(self.h, _p(buf), n, C.byref(carry), C.byref(nf),
                                                             C.byref(ef), C.byref(ec), C.byref(ed)))
        self._staged_len = sum(len(c) for c in wire) if isinstance(wire, (list, tuple)) else n
        rows = int(nf.value) + (1 if ec.value in (ERR_CHANGE, ERR_REQUIRED) else 0)
        if block:
            names = ["payload_off", "payload_len", "type"] + COLS32 + COLS64 + ["flags"] + (["key_hash"] if key_hash else [])
            dt = {"payload_off": np.uint64, "payload_len": np.uint32, "type": np.uint8, "flags": np.uint8,
                  "key_hash": np.uint64, **{k: np.uint32 for k in COLS32}, **{k: np.uint64 for k in COLS64}}
            if f64:
                dt.update({k: np.float64 for k in ["payload_off"] + COLS64})
            offs, at = [], 0
            for k in names:
                offs.append(at)
                at += (rows * np.dtype(dt[k]).itemsize + 8 + 63) & ~63
            blk = np.full(at + 64, 0xAB, np.uint8)
            col_off = (U64 * 14)(*(offs + [~0 & 0xFFFFFFFFFFFFFFFF] * (14 - len(offs))))
            if f64:
                _chk("drp_decode_fetch_block_ex", self.L.drp_decode_fetch_block_ex(self.h, _p(blk), at, col_off, 0, rows, 1))
            else:
                _chk("drp_decode_fetch_block", self.L.drp_decode_fetch_block(self.h, _p(blk), at, col_off, 0, rows))
            o = {k: blk[a:a + rows * np.dtype(dt[k]).itemsize].view(dt[k]) for k, a in zip(names, offs)}
            pieces = 0
        else:
            o = alloc_host_outputs(rows, key_hash)
        bounds = np.linspace(0, rows, pieces + 1).astype(np.int64)
        for a, b in zip(bounds[:-1], bounds[1:]):
            part = {k: v[a:] for k, v in o.items()}
            fr, co = _structs(part, _p)
            _chk("drp_decode_fetch", self.L.drp_decode_fetch(self.h, C.byref(fr), C.byref(co), int(a), int(b - a)))
        if keys:
            kp = np.zeros(max(rows, 1), np.uint32)
            tl = U64()
            rc = self.L.drp_decode_fetch_keys(self.h, 0, rows, _p(kp), None, 0, C.byref(tl))
            if rc == -1:  # DRP_E_INVAL: staged in pieces
                o.update(kp=None, key_text=None)
            else:
                _chk("drp_decode_fetch_keys", rc)
                text = np.zeros(max(int(tl.value), 1), np.uint8)
                _chk("drp_decode_fetch_keys", self.L.drp_decode_fetch_keys(self.h, 0, rows, _p(kp), _p(text),
                                                                           int(tl.value), C.byref(tl)))
                o.update(kp=kp[:rows], key_text=text[:int(tl.value)].tobytes())
        o.update(nframes=int(nf.value), err_frame=int(ef.value), err_code=int(ec.value), err_detail=int(ed.value),
                 consumed=int(carry.consumed), tail=int(carry.tail_kind), blob_remaining=int(carry.blob_remaining),
                 frame_bytes=int(carry.frame_bytes))
        return o

    # ---- the asynchronous calls: device pointers, launched on this ctx's stream --------------------
    def _call(self, fn, ref, *args):
        """One asynchronous call of the C function `fn` (ctx first, then args): this ctx's stream is
        ordered after torch's before it and torch's after this ctx's behind it, on the device of the
        tensor `ref` (None: no ordering)."""
        if ref is not None:
            self.order_after_torch(ref)
        _chk(fn, getattr(self.L, fn)(self.h, *args))
        if ref is not None:
            self.order_torch_after(ref)

    # ---- device decode over torch tensors (bench path) --------------------------------
    def decode_device(self, wire_t, stream_off_t, entry_t, outs, cap, results_t):
        """All arguments are torch CUDA tensors (uint8 wire, int64 offsets); outs is a dict
        of column tensors; results_t is a uint8 tensor of nstreams*sizeof(StreamResult)."""
        fr, co = _structs(outs, _tp)
        self._call("drp_decode_device", wire_t, _tp(wire_t), wire_t.numel(), _tp(stream_off_t), _tp(entry_t),
                   stream_off_t.numel() - 1, C.byref(fr), C.byref(co), cap, _tp(results_t))

    # ---- encode -----------------------------------------------------------------------
    def encode_device(self, cols_t, heap_t, n, frame_off_t, out_t, cap):
        """Device encode over torch CUDA tensors (asynchronous, on this ctx's stream): cols_t
        holds the drp_change_src columns (int64 offsets, int32 lengths, int64 numbers, uint8
        flags); frame_off_t (int64, n + 1) receives the frame offsets, out_t (uint8) the wire."""
        self._call("drp_encode_device", heap_t, C.byref(_src(cols_t)), _tp(heap_t), heap_t.numel(), n,
                   _tp(frame_off_t), _tp(out_t), cap)

    def encode_batch(self, heap, cols):
        n = len(cols["key_len"])
        h = np.frombuffer(bytes(heap), np.uint8) if not isinstance(heap, np.ndarray) else heap
        src = _src({k: np.ascontiguousarray(cols[k]) for k in SRC_COLS}, _p)
        total = U64()
        _chk("drp_encode_size", self.L.drp_encode_size(self.h, C.byref(src), n, C.byref(total)))
        out = np.zeros(max(16, int(total.value)), np.uint8)
        written = U64()
        hb = h if h.size else np.zeros(16, np.uint8)
        _chk("drp_encode_batch", self.L.drp_encode_batch(self.h, C.byref(src), _p(hb), int(h.size), n,
                                                         _p(out), int(total.value), C.byref(written)))
        return out[:int(written.value)].tobytes()

    # ---- select + re-encode (relay) ---------------------------------------------------
    def select_device(self, wire_t, cols, n, filter, out_rows, sel_idx_t, n_selected_t, _fn="drp_select_device"):
        """drp_select_device over torch CUDA tensors (asynchronous, on this ctx's stream): cols
        holds the decoded columns (payload_off, type and the Change columns, as decode_device
        wrote them), out_rows the drp_change_src columns to fill (n entries each: int64 offsets
        and numbers, int32 lengths, uint8 flags), sel_idx_t (int64, n entries) may be None,
        n_selected_t is an int64 tensor of one element."""
        self._call(_fn, wire_t, *_batch(wire_t, cols, n), _ref(filter), _ref(_src(out_rows)), _tp(sel_idx_t),
                   _tp(n_selected_t))

    def relay_staged(self, filter=None, cap=None, out=None, _fn="drp_relay_staged"):
        """drp_relay_staged over the batch last staged (decode_staged): returns (wire_bytes,
        n_selected). cap=None: the staged batch's length, which is always enough (the canonical
        encoding of a Change is never longer than the one received), so one call does it. A given
        cap that is too small raises DrpError(DRP_E_CAPACITY) with .written = the size needed.
        out: a host uint8 array to write into (at least cap bytes)."""
        written, nsel = U64(), U64()
        if cap is None:
            cap = getattr(self, "_staged_len", 0)
        buf = out if out is not None else np.zeros(max(16, cap), np.uint8)
        rc = getattr(self.L, _fn)(self.h, _ref(filter), _p(buf), cap, C.byref(written), C.byref(nsel))
        _chk(_fn, rc, written=int(written.value))
        return buf[:int(written.value)].tobytes(), int(nsel.value)

    # ---- latest per key (relay fan-in) ---------------------------------------------------
    def latest_device(self, wire_t, cols, n, filter, out_rows, sel_idx_t, n_selected_t):
        """drp_latest_device: select_device's arguments; of the rows the filter keeps, the one with
        the greatest change per (subset, key), in row order."""
        self.select_device(wire_t, cols, n, filter, out_rows, sel_idx_t, n_selected_t, _fn="drp_latest_device")

    def latest_staged(self, filter=None, cap=None, out=None):
        """drp_latest_staged over the batch last staged: relay_staged's arguments, results and
        errors, for the latest Change per (subset, key). cap=None: the staged batch's length, which
        is always enough (the winners are a subset of what relay_staged encodes)."""
        return self.relay_staged(filter, cap, out, _fn="drp_latest_staged")

    def set_latest_hash_mask(self, mask):
        """Test hook: the row hash of latest_device / latest_staged is ANDed with mask before it
        picks a slot (default all ones); results are identical for every mask."""
        _chk("drp_set_latest_hash_mask", self.L.drp_set_latest_hash_mask(self.h, mask & 0xFFFFFFFFFFFFFFFF))

    # ---- fan-out: many filters over one batch --------------------------------------------
    def fanout_device(self, wire_t, cols, n, filters, out_rows, rows_cap, sel_idx_t, row_base_t, splice=None):
        """drp_fanout_device over torch CUDA tensors (asynchronous, on this ctx's stream): cols and
        out_rows as select_device takes them (out_rows and sel_idx_t, which may be None, hold
        rows_cap entries), filters a list of make_filter results (None: keep every Change),
        row_base_t an int64 tensor of len(filters) + 1 entries. splice: None, or a dict of int64
        tensors blob_row (blob_cap entries), blob_rank (len(filters) * blob_cap) and n_blobs (1)."""
        sp = None
        if splice is not None:
            sp = Splice(_tp(splice["blob_row"]), _tp(splice["blob_rank"]), _tp(splice["n_blobs"]),
                        splice["blob_row"].numel() if splice["blob_row"] is not None else 0)
        self._call("drp_fanout_device", wire_t, *_batch(wire_t, cols, n), filter_array(filters), len(filters),
                   _ref(_src(out_rows)), rows_cap, _tp(sel_idx_t), _tp(row_base_t), _ref(sp))

    def fanout_staged(self, filters, cap=None, splice=False, out=None, blob_cap=None, _fn="drp_fanout_staged"):
        """drp_fanout_staged over the batch last staged (decode_staged), filters a list of
        make_filter results (None: keep every Change): returns ([wire bytes per filter],
        [n_selected per filter], splice_or_None). cap=None: len(filters) times the staged batch's
        length, which is always enough. A given cap that is too small raises
        DrpError(DRP_E_CAPACITY) with .written = the size needed and .n_selected. splice=True: a
        dict of n_blobs (the true count), blob_row (u64 per blob: its row as decode_staged numbers
        them) and blob_pos (u64 [len(filters)][blobs]: its byte offset within each output), the two
        arrays None when n_blobs exceeds blob_cap (None: as many as the staged batch can hold); raw:
        the two arrays as they were passed to the library.
        out: a host uint8 array to write into (at least cap bytes)."""
        K = len(filters)
        if cap is None:
            cap = K * getattr(self, "_staged_len", 0)
        buf = out if out is not None else np.zeros(max(16, cap), np.uint8)
        out_off, nsel = np.zeros(K + 1, np.uint64), np.zeros(max(K, 1), np.uint64)
        brow = bpos = nbl = None
        if splice:
            if blob_cap is None:
                blob_cap = getattr(self, "_staged_len", 0) // 2 + 1  # (a blob frame is at least two bytes)
            brow = np.full(max(blob_cap, 1), 0x5555555555555555, np.uint64)
            bpos = np.full(max(K * blob_cap, 1), 0x5555555555555555, np.uint64)
            nbl = np.zeros(1, np.uint64)
        args = (self.h, filter_array(filters), K, _p(buf), cap, _p(out_off), _p(nsel),
                _p(brow), _p(bpos), blob_cap or 0, _p(nbl))
        fn = getattr(self.L, _fn)  # (drp_fanout_latest_staged takes no blob arguments)
        _chk(_fn, fn(*args[:len(fn.argtypes)]), written=int(out_off[K]) if K <= FANOUT_MAX else 0,
             n_selected=[int(v) for v in nsel[:K]])
        outs = [buf[int(out_off[f]):int(out_off[f + 1])].tobytes() for f in range(K)]
        sp = None
        if splice:
            nb = int(nbl[0])
            fits = nb <= blob_cap
            sp = {"n_blobs": nb, "blob_row": brow[:nb].copy() if fits else None,
                  "blob_pos": bpos[:K * blob_cap].reshape(K, blob_cap)[:, :nb].copy() if fits else None,
                  "raw": (brow, bpos)}
        return outs, [int(v) for v in nsel[:K]], sp

    # ---- fan-out of latest per key: many snapshots over one grouping -----------------------
    def fanout_latest_device(self, wire_t, cols, n, filters, out_rows, rows_cap, sel_idx_t, row_base_t):
        """drp_fanout_latest_device: fanout_device's arguments without the splice; output f holds
        what latest_device gives for filters[f]."""
        self._call("drp_fanout_latest_device", wire_t, *_batch(wire_t, cols, n), filter_array(filters), len(filters),
                   _ref(_src(out_rows)), rows_cap, _tp(sel_idx_t), _tp(row_base_t))

    def fanout_latest_staged(self, filters, cap=None, out=None):
        """drp_fanout_latest_staged over the batch last staged (decode_staged), filters a list of
        make_filter results (None: every Change is a candidate): returns ([wire bytes per filter],
        [winners per filter]), output f being latest_staged's for filters[f]. cap=None: len(filters)
        times the staged batch's length, which is always enough. A given cap that is too small
        raises DrpError(DRP_E_CAPACITY) with .written = the size needed and .n_selected.
        out: a host uint8 array to write into (at least cap bytes)."""
        return self.fanout_staged(filters, cap, False, out, _fn="drp_fanout_latest_staged")[:2]

    def set_fanout_latest_pass(self, t):
        """Test hook: the filters one reduction pass of fanout_latest_device / fanout_latest_staged
        handles (0: the default); results are identical for every value."""
        _chk("drp_set_fanout_latest_pass", self.L.drp_set_fanout_latest_pass(self.h, t))

    # ---- store: the latest Change per key, resident on the device ---------------------------
    def store_init(self, store):
        """drp_store_init: an empty store (asynchronous)."""
        self._call("drp_store_init", store.arena, C.byref(store.desc()))

    def store_merge_device(self, store, wire_t, cols, n, filter=None):
        """drp_store_merge_device: merge the decoded rows [0, n) of a batch (wire_t and cols as
        latest_device takes them) into the store. Asynchronous; a merge that does not fit is refused on
        the device (store_query(...).refused)."""
        self._call("drp_store_merge_device", wire_t, C.byref(store.desc()), *_batch(wire_t, cols, n), _ref(filter))

    def store_merge_staged(self, store, filter=None, _fn="drp_store_merge_staged"):
        """drp_store_merge_staged over the batch last staged (decode_staged): returns the StoreInfo
        record; a refused merge raises DrpError(DRP_E_CAPACITY) with .info = the record."""
        info = StoreInfo()
        self.order_after_torch(store.arena)
        _chk(_fn, getattr(self.L, _fn)(self.h, C.byref(store.desc()), _ref(filter), C.byref(info)), info=info)
        return info

    # ---- merge report: per-row outcomes, the news view and the stale reply -----------------------
    def store_merge_report_device(self, store, wire_t, cols, n, filter=None, outcome_t=None, news_type_t=None,
                                  reply_rows=None, reply_idx_t=None, n_reply_t=None, reply_cap=0, flags=0,
                                  report=True):
        """drp_store_merge_report_device: store_merge_device's arguments and merge, and the report's
        outputs (all optional, uint8 / int64 CUDA tensors): outcome_t and news_type_t of n entries,
        reply_rows a dict of drp_change_src columns and reply_idx_t of reply_cap entries, n_reply_t of
        one. flags: REPORT_KEEP_BLOBS. report=False passes a NULL report. Asynchronous."""
        rep = None
        if report:
            dst = _src(reply_rows)
            rep = MergeReport(flags, 0, _tp(outcome_t), _tp(news_type_t), C.pointer(dst) if dst is not None else None,
                              _tp(reply_idx_t), _tp(n_reply_t), reply_cap, 0)
        self._call("drp_store_merge_report_device", wire_t, C.byref(store.desc()), *_batch(wire_t, cols, n),
                   _ref(filter), _ref(rep))

    def store_merge_news_staged(self, store, filter=None):
        """drp_store_merge_news_staged: store_merge_staged's arguments, result and errors; the ctx
        keeps the merge's news column (blobs kept) for fanout_news_staged."""
        return self.store_merge_staged(store, filter, _fn="drp_store_merge_news_staged")

    def fanout_news_staged(self, filters, cap=None, splice=False, out=None, blob_cap=None):
        """drp_fanout_news_staged: fanout_staged's arguments, results and errors, over the Changes of
        the staged batch that the last store_merge_news_staged found to be news (and its blobs)."""
        return self.fanout_staged(filters, cap, splice, out, blob_cap, _fn="drp_fanout_news_staged")

    # ---- lookup: a read-only probe of the store by key --------------------------------------------
    def store_lookup_device(self, store, wire_t, cols, n, filter=None, emit_mask=0, verdict_t=None, hit_row_t=None,
                            counts_t=None, lack_type_t=None, out_rows=None, out_query_t=None, n_out_t=None, rows_cap=0,
                            flags=0, lookup=True):
        """drp_store_lookup_device: the candidates among the rows [0, n) of (wire_t, cols), as
        latest_device takes them, looked up in the store by identity; nothing of the store is
        written. Outputs (all optional CUDA tensors): verdict_t (uint8) and hit_row_t (int64) of n
        entries, counts_t (int64, 5), lack_type_t (uint8, max_keys), out_rows a dict of
        drp_change_src columns and out_query_t (int64) of rows_cap entries, n_out_t (int64, 1).
        emit_mask: lookup_bit of LOOKUP_BEHIND / LEVEL / AHEAD. lookup=False passes a NULL drp_lookup.
        Asynchronous."""
        lk = None
        if lookup:
            dst = _src(out_rows)
            lk = Lookup(flags, emit_mask, _tp(verdict_t), _tp(hit_row_t), _tp(counts_t), _tp(lack_type_t),
                        C.pointer(dst) if dst is not None else None, _tp(out_query_t), _tp(n_out_t), rows_cap, 0, 0)
        self._call("drp_store_lookup_device", wire_t, C.byref(store.desc()), *_batch(wire_t, cols, n), _ref(filter),
                   _ref(lk))

    def store_lookup_staged(self, store, filter=None, reply=LOOKUP_FOUND, cap=None, out=None):
        """drp_store_lookup_staged over the batch last staged (decode_staged): returns (wire bytes,
        rows in them, [the five verdict counts]). reply: an emit_mask (the store's rows of the queries
        with those verdicts, in batch-row order) or LOOKUP_REPLY_LACK (every store row the sender of
        the staged have-list lacks, in store order). cap=None: first a call that only sizes the
        reply, then one with that capacity. A given cap that is too small raises
        DrpError(DRP_E_CAPACITY) with .written = the size needed. out: a host uint8 array to write
        into (at least cap bytes)."""
        written, nrows, counts = U64(), U64(), (U64 * 5)()
        self.order_after_torch(store.arena)
        call = lambda b, c: self.L.drp_store_lookup_staged(self.h, C.byref(store.desc()), _ref(filter), reply, _p(b), c,
                                                           C.byref(written), C.byref(nrows), counts)
        if cap is None:
            rc = call(None, 0)  # (sizes the reply: DRP_E_CAPACITY unless it is empty)
            if rc != DRP_E_CAPACITY:
                _chk("drp_store_lookup_staged", rc)
            cap = int(written.value)
        buf = out if out is not None else np.zeros(max(16, cap), np.uint8)
        _chk("drp_store_lookup_staged", call(buf, cap), written=int(written.value))
        return buf[:int(written.value)].tobytes(), int(nrows.value), [int(v) for v in counts]

    def store_compact(self, store, arena2_t, arena2_bytes=None):
        """drp_store_compact into arena2_t (a uint8 CUDA tensor). Asynchronous; the caller checks
        store_query(...).refused and, if 0, sets store.arena = arena2_t. arena2_bytes: the size to
        pass where it is not arena2_t's (0 for the one-byte stand-in of an empty arena)."""
        self._call("drp_store_compact", arena2_t, C.byref(store.desc()), _tp(arena2_t),
                   arena2_t.numel() if arena2_bytes is None else int(arena2_bytes))

    def store_query(self, store):
        """drp_store_query: waits for the ctx's stream and returns the StoreInfo record."""
        info = StoreInfo()
        _chk("drp_store_query", self.L.drp_store_query(self.h, C.byref(store.desc()), C.byref(info)))
        return info

    # ---- store lifecycle: load distinct rows, rehash ----------------------------------------------
    def store_load_device(self, store, wire_t, cols, n, filter=None, clash_t=None):
        """drp_store_load_device: the rows select_device selects from [0, n) of (wire_t, cols) enter
        the store as new rows, ungrouped and not looked up: the caller promises that their identities
        are distinct and not in the store. clash_t (int64, 1, optional) receives the rows that broke
        the promise; a store with clash > 0 must be dropped. Asynchronous; refused on the device as a
        merge is (store_query(...).refused)."""
        self._call("drp_store_load_device", wire_t, C.byref(store.desc()), *_batch(wire_t, cols, n), _ref(filter),
                   _tp(clash_t))

    def store_rehash_device(self, store, report_t=None):
        """drp_store_rehash_device: the store's table rebuilt from its rows in use under the ctx's
        current hash mask. report_t (int64, 2, optional): the rows left out as invalid, and the rows
        that share their identity with an earlier one; store_query(...).refused is 1 if either is
        nonzero. Asynchronous."""
        self._call("drp_store_rehash_device", store.arena, C.byref(store.desc()), _tp(report_t))

    # ---- ordered catch-up: a fan-out's outputs in change order, with a per-peer limit -------------
    def order_device(self, rows, row_base_t, nseg, rows_cap, out_rows, out_base_t, limit=None, keep_ties=False,
                     sel_idx_t=None, out_sel_idx_t=None, flags=None):
        """drp_order_device over torch CUDA tensors (asynchronous, on this ctx's stream): rows and
        row_base_t (int64, nseg + 1) as fanout_device / fanout_latest_device leave them, out_rows a
        second set of drp_change_src columns of rows_cap entries, out_base_t (int64, nseg + 1) the
        bounds of the outputs. Output f holds the rows of segment f in ascending change (unsigned,
        ties in input order), cut to limit[f] rows (limit: None, one int for every segment, or a list;
        an entry of None or 2**64 - 1: no limit); keep_ties: a cut inside a run of equal change moves
        to the run's end. out_sel_idx_t receives sel_idx_t in the same order (both int64, rows_cap
        entries). flags overrides the flag word (tests of the error returns)."""
        lim = None
        if limit is not None:
            vals = [limit] * nseg if isinstance(limit, int) else list(limit)
            lim = (U64 * max(1, len(vals)))(*[0xFFFFFFFFFFFFFFFF if v is None else int(v) for v in vals])
        fl = (ORDER_KEEP_TIES if keep_ties else 0) if flags is None else flags
        ref = next((t for t in (row_base_t, out_base_t) if t is not None), None)
        self._call("drp_order_device", ref, _ref(_src(rows)), _tp(row_base_t), nseg, rows_cap, lim, fl,
                   _ref(_src(out_rows)), _tp(sel_idx_t), _tp(out_sel_idx_t), _tp(out_base_t))

    # ---- key-ordered listing: a fan-out's outputs in key order, with a key range and a page --------
    def order_keys_device(self, heap_t, rows, row_base_t, nseg, rows_cap, out_rows, out_base_t, pages=None,
                          keep_ties=False, sel_idx_t=None, out_sel_idx_t=None, totals_t=None, flags=None):
        """drp_order_keys_device over torch CUDA tensors (on this ctx's stream; the call waits for the
        stream once inside): heap_t the uint8 tensor the rows' offsets point into (None: no heap),
        rows, row_base_t, out_rows, out_base_t, sel_idx_t and out_sel_idx_t as order_device takes them.
        Output f holds the rows of segment f in ascending (key bytes, subset absent first, subset
        bytes, input position), restricted to pages[f]'s key range and cut to its limit (pages: None,
        or a list of make_key_page results / None per segment); keep_ties: a cut inside a run of equal
        key moves to the run's end. totals_t (int64, 2, optional): the rows that took part, and the
        rows left out (a range outside the heap, or a key or subset above KEYORDER_MAX_BYTES). flags
        overrides the flag word (tests of the error returns)."""
        pg = key_page_array(list(pages)) if pages is not None else None
        fl = (KEYORDER_KEEP_TIES if keep_ties else 0) if flags is None else flags
        ref = next((t for t in (row_base_t, out_base_t, heap_t) if t is not None), None)
        self._call("drp_order_keys_device", ref, _tp(heap_t), heap_t.numel() if heap_t is not None else 0,
                   _ref(_src(rows)), _tp(row_base_t), nseg, rows_cap, pg, fl, _ref(_src(out_rows)), _tp(sel_idx_t),
                   _tp(out_sel_idx_t), _tp(out_base_t), _tp(totals_t))

    # ---- digest / reconcile: what differs between two stores ------------------------------------
    def digest_device(self, wire_t, cols, n, filter, bits, cells_t, totals_t=None):
        """drp_digest_device over torch CUDA tensors (asynchronous, on this ctx's stream): wire_t and
        cols as select_device takes them; cells_t an int64 tensor of 2**bits * 2 elements (count, sum
        per bucket), zeroed and filled; totals_t (int64, two elements, may be None): the rows
        digested, and the selected rows left out for a range outside the wire."""
        self._call("drp_digest_device", wire_t, *_batch(wire_t, cols, n), _ref(filter), bits, _tp(cells_t),
                   _tp(totals_t))

    def digest_diff_device(self, a_t, b_t, bits, bucket_set_t, n_diff_t):
        """drp_digest_diff_device: a_t, b_t two digests of 2**bits cells; bucket_set_t (int64,
        max(1, 2**bits // 64) words) gets bit b set iff cell b differs, n_diff_t (int64, one element)
        the number of such buckets. Asynchronous."""
        self._call("drp_digest_diff_device", a_t, _tp(a_t), _tp(b_t), bits, _tp(bucket_set_t), _tp(n_diff_t))

    def select_buckets_device(self, wire_t, cols, n, filter, bits, bucket_set_t, out_rows, sel_idx_t, n_selected_t):
        """drp_select_buckets_device: select_device's arguments and outputs, for the rows
        digest_device counted (same filter, same bits) in the buckets whose bit is set in
        bucket_set_t."""
        self._call("drp_select_buckets_device", wire_t, *_batch(wire_t, cols, n), _ref(filter), bits,
                   _tp(bucket_set_t), _ref(_src(out_rows)), _tp(sel_idx_t), _tp(n_selected_t))

    # ---- refined digests: a second level inside the differing buckets ----------------------------
    def digest_refine_device(self, wire_t, cols, n, filter, bits, bucket_set_t, sub_bits, cells2_t, cells_cap, totals_t):
        """drp_digest_refine_device: digest_device's candidates in the buckets whose bit is set in
        bucket_set_t (int64, max(1, 2**bits // 64) words), summed into cells2_t (int64, cells_cap * 2
        elements) at cell slot(bucket) << sub_bits | sub. totals_t (int64, three elements, required):
        the rows digested, the selected rows left out for a range outside the wire, n_set. The cells
        are written only if n_set << sub_bits <= cells_cap; totals_t is complete either way."""
        self._call("drp_digest_refine_device", wire_t, *_batch(wire_t, cols, n), _ref(filter), bits,
                   _tp(bucket_set_t), sub_bits, _tp(cells2_t), cells_cap, _tp(totals_t))

    def digest_diff_cells_device(self, a_t, b_t, ncells, cell_set_t, n_diff_t):
        """drp_digest_diff_cells_device: digest_diff_device for any cell count; cell_set_t (int64,
        max(1, ceil(ncells / 64)) words), n_diff_t (int64, one element). Asynchronous."""
        self._call("drp_digest_diff_cells_device", a_t, _tp(a_t), _tp(b_t), ncells, _tp(cell_set_t), _tp(n_diff_t))

    def select_refined_device(self, wire_t, cols, n, filter, bits, bucket_set_t, sub_bits, cell_set_t, out_rows,
                              sel_idx_t, n_selected_t):
        """drp_select_refined_device: select_buckets_device's arguments and outputs, for the rows
        digest_refine_device counted (same filter, bits, bucket set and sub_bits) in the cells whose
        bit is set in cell_set_t."""
        self._call("drp_select_refined_device", wire_t, *_batch(wire_t, cols, n), _ref(filter), bits,
                   _tp(bucket_set_t), sub_bits, _tp(cell_set_t), _ref(_src(out_rows)), _tp(sel_idx_t),
                   _tp(n_selected_t))


_SIGNED = {8: np.int64, 4: np.int32, 1: np.uint8}  # (torch's dtypes for the 64-, 32- and 8-bit columns)


def _upload(a, dev):
    """A numpy array as a tensor on dev, its unsigned 64- and 32-bit entries as the signed dtype torch has."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype.itemsize])).to(dev)


class Store:
    """A drp_store in torch tensors on `device`: the arena, the frame and Change columns (max_keys
    entries each), the identity table and the info record. The columns (self.cols) and the arena are
    a decoded batch: any *_device relay call of the ctx runs over (store.arena, store.cols,
    n = max_keys) as it does over a decoded wire."""

    def __init__(self, ctx, max_keys, arena_bytes, device="cuda:0"):
        import torch
        self.ctx, self.max_keys = ctx, int(max_keys)
        dev = torch.device(device)
        z = lambda n, dt: torch.zeros(max(int(n), 1), dtype=dt, device=dev)
        self.arena = z(arena_bytes, torch.uint8)
        self.arena_bytes = int(arena_bytes)
        self.cols = {"payload_off": z(max_keys, torch.int64), "payload_len": z(max_keys, torch.int32),
                     "type": z(max_keys, torch.uint8), "flags": z(max_keys, torch.uint8)}
        for k in COLS32:
            self.cols[k] = z(max_keys, torch.int32)
        for k in COLS64:
            self.cols[k] = z(max_keys, torch.int64)
        self.table = z(lib().drp_store_table_bytes(self.max_keys) // 8, torch.int64)
        self.info = z(C.sizeof(StoreInfo) // 8, torch.int64)
        ctx.store_init(self)

    def desc(self):
        fr, co = _structs(self.cols, _tp)
        return StoreDesc(_tp(self.arena), self.arena_bytes, fr, co, self.max_keys, _tp(self.table), _tp(self.info))

    def _view(self):
        return self.arena[:self.arena_bytes] if self.arena_bytes else self.arena[:0]

    def _zeros(self, n, dtype):
        import torch
        return torch.zeros(max(int(n), 1), dtype=dtype, device=self.arena.device)

    def _out_rows(self, cap):
        """A set of output rows: the ten drp_change_src columns, cap entries each, on the store's device."""
        import torch
        return {k: self._zeros(cap, torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else torch.int64)
                for k in SRC_COLS}

    def merge_device(self, wire_t, cols, n, filter=None):
        self.ctx.store_merge_device(self, wire_t, cols, n, filter)

    def merge_staged(self, filter=None):
        return self.ctx.store_merge_staged(self, filter)

    def query(self):
        return self.ctx.store_query(self)

    def merge_report(self, wire_t, cols, n, filter=None, keep_blobs=False, reply=False):
        """merge_device with the full report: {"outcome", "news_type"} (uint8 tensors of n entries:
        MERGE_* per batch row, and the type column under which the batch holds only its news), and,
        with reply=True (else None), {"reply_rows", "reply_idx", "n_reply"}: the store's rows for the
        batch's stale winners as drp_change_src columns over the arena, their store rows, and the
        count as an int64 tensor of one element (reply_cap = n). Asynchronous."""
        import torch
        z = self._zeros
        r = {"outcome": z(n, torch.uint8), "news_type": z(n, torch.uint8), "reply_rows": None, "reply_idx": None,
             "n_reply": None}
        if reply:
            r["reply_rows"], r["reply_idx"], r["n_reply"] = self._out_rows(n), z(n, torch.int64), z(1, torch.int64)
        self.ctx.store_merge_report_device(self, wire_t, cols, n, filter, r["outcome"], r["news_type"],
                                           r["reply_rows"], r["reply_idx"], r["n_reply"], n if reply else 0,
                                           REPORT_KEEP_BLOBS if keep_blobs else 0)
        r["outcome"], r["news_type"] = r["outcome"][:n], r["news_type"][:n]
        return r

    def _encode_outputs(self, rows, base, heap_t, K):
        """One encode_device of fan-out rows (bounds base: a tensor, or its entries as a list; K
        outputs) over heap_t: [bytes per output]."""
        import torch
        rb = base if isinstance(base, list) else [int(v) for v in base.cpu()]  # (torch's stream was ordered after the ctx's)
        total = rb[K]
        if total == 0:
            return [b""] * K
        need = U64()
        _chk("drp_encode_size", self.ctx.L.drp_encode_size(self.ctx.h, C.byref(_src(rows)), total, C.byref(need)))
        foff = self._zeros(total + 1, torch.int64)
        out = self._zeros(need.value, torch.uint8)
        self.ctx.encode_device(rows, heap_t, total, foff, out, int(need.value))
        fo, o = foff.cpu().numpy(), out.cpu().numpy()
        return [o[int(fo[rb[f]]):int(fo[rb[f + 1]])].tobytes() for f in range(K)]

    def _encode_rows(self, rows, n_t):
        """One encode_device of rows [0, n_t[0]) (n_t: an int64 tensor on the device) with the arena as
        the heap: their bytes."""
        import torch
        base = torch.cat([self._zeros(1, torch.int64), n_t[:1]])
        return self._encode_outputs(rows, base, self._view(), 1)[0]

    def relay_news(self, wire_t, cols, n, filters, merge_filter=None):
        """The hub step: one merge with a report, one fanout_device over the batch with the report's
        news_type as its type column, one encode_device with the wire as the heap. Returns (info,
        [wire bytes per filter]): output f holds the batch's Changes that changed the store and pass
        filters[f], in batch-row order."""
        import torch
        news = self._zeros(n, torch.uint8)
        self.ctx.store_merge_report_device(self, wire_t, cols, n, merge_filter, None, news, flags=REPORT_KEEP_BLOBS)
        K = len(filters)
        cap = K * int(n)
        rows, base = self._out_rows(cap), self._zeros(K + 1, torch.int64)
        self.ctx.fanout_device(wire_t, dict(cols, type=news), n, filters, rows, cap, None, base)
        outs = self._encode_outputs(rows, base, wire_t, K)
        return self.query(), outs

    def reply_bytes(self, report):
        """The bytes to send back to the peer whose batch merge_report(..., reply=True) merged: one
        encode_device of the reply rows with the arena as the heap."""
        if report.get("n_reply") is None:
            raise ValueError("the report holds no reply (merge_report(..., reply=True))")
        return self._encode_rows(report["reply_rows"], report["n_reply"])

    def compact(self, arena2_bytes=None):
        """Compact into a fresh arena of arena2_bytes (default: the live bytes); returns the record.
        The store takes the new arena unless the compact was refused."""
        import torch
        if arena2_bytes is None:
            i = self.query()
            arena2_bytes = i.arena_used - i.arena_dead
        a2 = self._zeros(arena2_bytes, torch.uint8)
        # (arena2's true size is passed: the 1-byte stand-in for an empty arena holds nothing)
        self.ctx.store_compact(self, a2, int(arena2_bytes))
        i = self.query()
        if not i.refused:
            self.arena, self.arena_bytes = a2, int(arena2_bytes)
        return i

    # ---- lifecycle: grow, prune, save and restore -------------------------------------------------
    def _take(self, other):
        """This store becomes `other` (its tensors and sizes)."""
        for k in ["max_keys", "arena", "arena_bytes", "cols", "table", "info"]:
            setattr(self, k, getattr(other, k))

    def _rehash_checked(self):
        """One rehash with a report: DrpError if it names an invalid or a duplicate row."""
        import torch
        report = self._zeros(2, torch.int64)
        self.ctx.store_rehash_device(self, report)
        bad = [int(v) for v in report.cpu()]
        if any(bad):
            raise DrpError(f"drp_store_rehash_device (report {bad})", DRP_E_INVAL)

    def grow(self, max_keys=None, arena_bytes=None):
        """Resize the store in place: new column tensors and a new table for max_keys (the rows in use
        copied with torch, then one rehash), a new arena for arena_bytes (the bytes in use copied).
        No payload moves within the arena and the rows keep their index. ValueError for a size below
        what is in use; DrpError if the rehash reports an invalid or duplicate row (the store is left
        as it was). Returns the record."""
        import copy
        import torch
        i = self.query()
        mk = self.max_keys if max_keys is None else int(max_keys)
        ab = self.arena_bytes if arena_bytes is None else int(arena_bytes)
        if mk < max(int(i.rows), 1) or ab < int(i.arena_used):
            raise ValueError(f"grow({mk}, {ab}) below what is in use ({i.rows} rows, {i.arena_used} bytes)")
        dev = self.arena.device
        new = copy.copy(self)
        if ab != self.arena_bytes:
            new.arena = torch.zeros(max(ab, 1), dtype=torch.uint8, device=dev)
            new.arena[:i.arena_used] = self.arena[:i.arena_used]
            new.arena_bytes = ab
        if mk != self.max_keys:
            new.cols = {k: torch.zeros(mk, dtype=v.dtype, device=dev) for k, v in self.cols.items()}
            for k, v in self.cols.items():
                new.cols[k][:i.rows] = v[:i.rows]
            new.table = torch.zeros(lib().drp_store_table_bytes(mk) // 8, dtype=torch.int64, device=dev)
            new.max_keys = mk
            try:
                new._rehash_checked()
            except DrpError:
                self.ctx.store_rehash_device(self)  # (the shared record's last-merge group, and this table)
                raise
        self._take(new)
        return self.query()

    def retain(self, filter=None, type_t=None, max_keys=None, arena_bytes=None):
        """Keep only the rows that select_device selects from the store's view under `filter`, with
        type_t (uint8, max_keys entries: a lookup's lack_type, the store's own type column with entries
        zeroed) in the type column's place: a fresh store (max_keys / arena_bytes, default the same
        sizes) and one store_load_device of the view into it, with the clash check. Returns the fresh
        store's record, with .clash = the check's count; this store takes the new tensors unless the
        load was refused or clashed. The kept rows are renumbered in their old order, the arena is
        compacted and arena_dead is 0."""
        import torch
        new = Store(self.ctx, self.max_keys if max_keys is None else max_keys,
                    self.arena_bytes if arena_bytes is None else arena_bytes, device=self.arena.device)
        view = self.cols if type_t is None else dict(self.cols, type=type_t)
        clash = self._zeros(1, torch.int64)
        self.ctx.store_load_device(new, self._view(), view, self.max_keys, filter, clash)
        i = new.query()
        i.clash = int(clash.cpu()[0])
        if not i.refused and not i.clash:
            self._take(new)
        return i

    def state(self):
        """The store as host numpy arrays: {"cols": {name: the column's rows [0, rows)}, "arena": the
        bytes [0, arena_used), "rows", "arena_used", "arena_dead", "merges"}. Store.from_state brings
        it back; the table is not saved (it is rebuilt from the rows)."""
        i = self.query()
        return {"cols": {k: v[:i.rows].cpu().numpy().copy() for k, v in self.cols.items()},
                "arena": self.arena[:i.arena_used].cpu().numpy().copy(),
                "rows": int(i.rows), "arena_used": int(i.arena_used), "arena_dead": int(i.arena_dead),
                "merges": int(i.merges)}

    @classmethod
    def from_state(cls, ctx, state, max_keys=None, arena_bytes=None, device="cuda:0"):
        """A store restored from Store.state(): allocate (default sizes: what the state uses), upload
        the columns, the arena and the record, and rehash with a report. ValueError for a state that
        does not fit the sizes or its own counts; DrpError if the rehash reports an invalid or
        duplicate row."""
        rows, used = int(state["rows"]), int(state["arena_used"])
        mk = max(rows, 1) if max_keys is None else int(max_keys)
        ab = used if arena_bytes is None else int(arena_bytes)
        if mk < rows or ab < used or len(state["arena"]) != used or used % 16 or int(state["arena_dead"]) > used:
            raise ValueError(f"the state ({rows} rows, {used} bytes) does not fit ({mk}, {ab})")
        s = cls(ctx, mk, ab, device=device)
        if set(state["cols"]) != set(s.cols) or any(len(v) != rows for v in state["cols"].values()):
            raise ValueError("the state's columns are not a store's, or not `rows` long")
        dev = s.arena.device
        for k, v in state["cols"].items():
            s.cols[k][:rows] = _upload(v, dev)
        s.arena[:used] = _upload(np.asarray(state["arena"], np.uint8), dev)
        rec = np.zeros(C.sizeof(StoreInfo) // 8, np.int64)
        rec[:4] = [rows, used, int(state["arena_dead"]), int(state["merges"])]
        s.info.copy_(_upload(rec, dev))
        s._rehash_checked()
        return s

    def lookup(self, wire_t, cols, n, filter=None, emit=(LOOKUP_BEHIND, LOOKUP_LEVEL, LOOKUP_AHEAD), lack=False):
        """store_lookup_device with the full set of outputs: {"verdict" (uint8, n entries: LOOKUP_*
        per batch row), "hit_row" (int64, n: the store row, -1 for NONE and ABSENT), "counts" (int64,
        5: rows per verdict)}; with emit (verdict codes; None or empty: no emission, the entries are
        None) {"out_rows", "out_query", "n_out"}: the store's rows of the queries with those verdicts
        as drp_change_src columns over the arena, their batch rows, and the count as an int64 tensor
        of one element (rows_cap = n); with lack=True (else None) "lack_type": the uint8 column of
        max_keys entries under which the store's view holds the rows the batch's sender lacks.
        Nothing of the store is written. Asynchronous."""
        import torch
        z = self._zeros
        r = {"verdict": z(n, torch.uint8), "hit_row": z(n, torch.int64), "counts": z(5, torch.int64),
             "lack_type": z(self.max_keys, torch.uint8) if lack else None, "out_rows": None, "out_query": None,
             "n_out": None}
        mask = 0
        for code in emit or ():
            mask |= lookup_bit(code)
        if mask:
            r["out_rows"], r["out_query"], r["n_out"] = self._out_rows(n), z(n, torch.int64), z(1, torch.int64)
        self.ctx.store_lookup_device(self, wire_t, cols, n, filter, mask, r["verdict"], r["hit_row"], r["counts"],
                                     r["lack_type"], r["out_rows"], r["out_query"], r["n_out"], n if mask else 0)
        r["verdict"], r["hit_row"] = r["verdict"][:n], r["hit_row"][:n]
        if lack:
            r["lack_type"] = r["lack_type"][:self.max_keys]
        return r

    def get(self, keys):
        """The multi-get: the store's current Change of each key. keys: a list of `key` or
        `(subset, key)` byte strings (a key occurring twice is answered twice). The queries are built
        here (key | subset end to end in one heap, type 1, change 0, no value: no wire, no decode);
        one lookup that emits every found row and one encode_device with the arena as the heap.
        Returns (hit_row, wire bytes): an int64 numpy array, the store row of each key or -1 where the
        store does not hold it, and the found rows in query order as change frames."""
        n = len(keys)
        dev = self.arena.device
        q = alloc_host_outputs(max(n, 1))
        heap = bytearray()
        for i, k in enumerate(keys):
            sub, key = k if isinstance(k, tuple) else (None, k)
            q["payload_off"][i], q["type"][i] = len(heap), TYPE_CHANGE
            q["key_len"][i], q["subset_off"][i] = len(key), len(key)
            heap += key
            if sub is not None:
                q["subset_len"][i], q["flags"][i] = len(sub), F_SUBSET
                heap += sub
            q["payload_len"][i] = len(heap) - int(q["payload_off"][i])
            q["value_off"][i] = q["payload_len"][i]
        cols = {k: _upload(v, dev) for k, v in q.items()}
        heap_t = _upload(np.frombuffer(bytes(heap) or b"\0", np.uint8).copy(), dev)[:len(heap)]
        r = self.lookup(heap_t, cols, n)
        return r["hit_row"].cpu().numpy().copy(), self._encode_rows(r["out_rows"], r["n_out"])

    def sync_reply(self, wire_t, cols, n, filter=None):
        """The answer to a have-list (wire_t, cols, n: a batch of Changes whose values do not matter,
        the sender's keys and versions): one lookup with lack_type, then the existing fan-out
        (fanout_rows) and encoder over the store's view with that column in the type column's place.
        Returns the bytes of the store's rows the sender lacks (those it did not name, and those it
        named with a smaller change), under `filter`, in store order."""
        r = self.lookup(wire_t, cols, n, emit=None, lack=True)
        rows, base = self.fanout_rows([filter], type_t=r["lack_type"])
        return self._encode_outputs(rows, base, self._view(), 1)[0]

    def fanout_rows(self, filters, n=None, rows_cap=None, type_t=None):
        """The existing fanout_device over the store's view, rows [0, n) (default max_keys: the rows
        past info.rows are no Changes). Returns (out_rows, row_base_t): drp_change_src columns of
        rows_cap entries (default len(filters) * n) and the int64 tensor of len(filters) + 1 bounds.
        type_t: a column to take the type column's place (lookup's lack_type). Asynchronous."""
        import torch
        n = self.max_keys if n is None else int(n)
        K = len(filters)
        cap = K * n if rows_cap is None else int(rows_cap)
        rows, base = self._out_rows(cap), self._zeros(K + 1, torch.int64)
        view = self.cols if type_t is None else dict(self.cols, type=type_t)
        self.ctx.fanout_device(self._view(), view, n, filters, rows, cap, None, base)
        return rows, base

    def fanout(self, filters, n=None):
        """The catch-up call: one fanout_device over the store and one encode_device with the arena
        as the heap. filters: make_filter results (peer f at version T: change_range=(T + 1,
        2**64 - 1), with its subset / key prefix). Returns [wire bytes per filter], in store order."""
        rows, base = self.fanout_rows(filters, n)
        return self._encode_outputs(rows, base, self._view(), len(filters))

    def _ordered(self, filters, n, order):
        """fanout_rows, then order(rows, base, K, total, out_rows, out_base) (one of the ctx's two
        orders), then one encode_device with the arena as the heap: (out_rows, the bounds of the
        outputs as a list, [bytes per output]), or None when nothing is to be sent."""
        import torch
        K = len(filters)
        rows, base = self.fanout_rows(filters, n)
        total = int(base.cpu()[K])  # (torch's stream was ordered after the ctx's)
        if total == 0:
            return None
        out_rows, out_base = self._out_rows(total), self._zeros(K + 1, torch.int64)
        order(rows, base, K, total, out_rows, out_base)
        ob = [int(v) for v in out_base.cpu()]
        if ob[K] == 0:
            return None
        return out_rows, ob, self._encode_outputs(out_rows, ob, self._view(), K)

    def catch_up(self, filters, limit=None, keep_ties=True, n=None):
        """The ordered catch-up: fanout_rows over the store, one order_device and one encode_device
        with the arena as the heap. filters as fanout takes them (peer f at version T: change_range=
        (T + 1, 2**64 - 1)); limit: None, one int for every peer, or a list (rows per page); keep_ties:
        a page never ends inside a run of equal change. Returns, per filter, (wire bytes, rows sent,
        last_change): the peer's rows in ascending change as change frames, their number, and the
        change of the last one (None for an empty page). The paging loop: send a page, the peer's new
        T is last_change, repeat until a page is empty."""
        import torch
        K = len(filters)
        got = self._ordered(filters, n, lambda *a: self.ctx.order_device(*a, limit=limit, keep_ties=keep_ties))
        if got is None:
            return [(b"", 0, None)] * K
        out_rows, ob, outs = got
        ends = [ob[f + 1] - 1 for f in range(K) if ob[f + 1] > ob[f]]
        last = out_rows["change"][torch.tensor(ends, dtype=torch.int64, device=self.arena.device)]
        last = dict(zip(ends, (int(v) for v in last.cpu().numpy().view(np.uint64))))
        return [(outs[f], ob[f + 1] - ob[f], last.get(ob[f + 1] - 1) if ob[f + 1] > ob[f] else None) for f in range(K)]

    def list_keys(self, filters, pages=None, keep_ties=True, n=None):
        """The key-ordered listing: fanout_rows over the store, one order_keys_device and one
        encode_device with the arena as the heap. filters as fanout takes them (the listing's subset,
        key prefix and version bound: subset=, subset_none=, key_prefix=, change_range=); pages: None,
        or per filter a make_key_page result or None (from_ / after / until bound the key, limit the
        rows of a page); keep_ties: a page never ends inside a run of equal key (the rows of one key
        under different subsets). Returns, per filter, (wire bytes, rows sent, last_key): the rows in
        ascending (key, subset) as change frames, their number, and the key of the last one (None for
        an empty page). Raises ValueError naming the count if rows were left out (a key or subset
        above KEYORDER_MAX_BYTES). The paging loop:

            after = None
            while True:
                wire, sent, last_key = store.list_keys(
                    [make_filter(key_prefix=b"users/")], [make_key_page(after=after, limit=500)])[0]
                if not sent:
                    break
                send(wire)
                after = last_key"""
        import torch
        K = len(filters)
        totals = self._zeros(2, torch.int64)

        def order(*a):
            self.ctx.order_keys_device(self._view(), *a, pages=pages, keep_ties=keep_ties, totals_t=totals)
            left = int(totals.cpu()[1])
            if left:
                raise ValueError(f"list_keys: {left} rows left out of the order (key or subset too long, or outside the arena)")

        got = self._ordered(filters, n, order)
        if got is None:
            return [(b"", 0, None)] * K
        out_rows, ob, outs = got
        ends = torch.tensor([ob[f + 1] - 1 for f in range(K) if ob[f + 1] > ob[f]], dtype=torch.int64,
                            device=self.arena.device)
        koff, klen = out_rows["key_off"][ends].cpu().tolist(), out_rows["key_len"][ends].cpu().tolist()
        last = {int(e): bytes(self.arena[o_:o_ + l_].cpu().numpy()) for e, o_, l_ in zip(ends.cpu().tolist(), koff, klen)}
        return [(outs[f], ob[f + 1] - ob[f], last[ob[f + 1] - 1] if ob[f + 1] > ob[f] else None) for f in range(K)]

    def digest(self, bits, filter=None, n=None):
        """The store's bucket digest (digest_device over its view, rows [0, n), default max_keys): an
        int64 tensor of shape (2**bits, 2) on the store's device, [b] = (count, sum) of bucket b, the
        16 bytes per bucket two hubs exchange. torch's stream is ordered after the ctx's."""
        import torch
        n = self.max_keys if n is None else int(n)
        cells = torch.zeros((1 << bits, 2), dtype=torch.int64, device=self.arena.device)
        self.ctx.digest_device(self._view(), self.cols, n, filter, bits, cells)
        return cells

    @staticmethod
    def _set_bits(words_t):
        """The increasing numbers of the bits set in an int64 tensor of words (numpy int64)."""
        w = words_t.cpu().numpy().view(np.uint8)
        return np.flatnonzero(np.unpackbits(w, bitorder="little")).astype(np.int64)

    def reconcile(self, peer_cells, bits, filter=None):
        """What this store holds in the buckets where its digest differs from a peer's: digest, diff
        and bucket select over the view with n = max_keys, and one encode_device with the arena as the
        heap (as fanout). peer_cells: the peer's digest(bits, filter), a tensor or a numpy array of
        2**bits * 2 64-bit words. Returns (wire bytes, differing buckets): the rows in store order as
        change frames, for the peer to decode and merge, and the increasing bucket numbers (numpy
        int64) in which the two digests differ."""
        import torch
        peer = self._set_tensor(peer_cells)
        if peer.numel() != 2 << bits:
            raise ValueError(f"peer_cells holds {peer.numel()} words, 2**{bits} cells are {2 << bits}")
        mine = self.digest(bits, filter)
        bset = self._zeros((1 << bits) // 64, torch.int64)
        cnt = self._zeros(2, torch.int64)  # [0] differing buckets, [1] rows selected
        self.ctx.digest_diff_device(mine, peer, bits, bset, cnt[0:1])
        rows = self._out_rows(self.max_keys)
        self.ctx.select_buckets_device(self._view(), self.cols, self.max_keys, filter, bits, bset, rows, None, cnt[1:2])
        return self._encode_rows(rows, cnt[1:2]), self._set_bits(bset)

    def _set_tensor(self, words):
        """A bit set (a tensor or a numpy array of 64-bit words) as an int64 tensor on the store's device."""
        import torch
        if not isinstance(words, torch.Tensor):
            words = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy())
        return words.to(device=self.arena.device, dtype=torch.int64).contiguous()

    def digest_refined(self, bits, bucket_set, sub_bits, filter=None):
        """The second level of the store's digest inside the buckets of bucket_set (a tensor or a numpy
        array of max(1, 2**bits // 64) words, as digest_diff_device writes it): (cells2, n_set), cells2
        an int64 tensor of shape (n_set << sub_bits, 2) on the store's device, [slot << sub_bits | sub]
        = (count, sum) of the rows of the slot-th set bucket whose next sub_bits hash bits are sub.

        The exchange: both hubs hold both first-level digests (each sent its digest(bits)), so both
        derive the same bucket_set from one diff; each then sends its cells2, and each encodes its rows
        of the differing cells (reconcile_refined). The sub-cells of a slot add up to the first-level
        cell of that bucket. n_set is the popcount of the set, taken on the host to size the tensor."""
        import torch
        bset = self._set_tensor(bucket_set)
        words = max(1, (1 << bits) // 64)
        if bset.numel() != words:
            raise ValueError(f"bucket_set holds {bset.numel()} words, 2**{bits} buckets are {words}")
        w = bset.cpu().numpy().view(np.uint64)
        if bits < 6:
            w = w & np.uint64((1 << (1 << bits)) - 1)
        ncells = int(np.unpackbits(w.view(np.uint8)).sum()) << sub_bits
        dev = self.arena.device
        cells2 = torch.zeros((max(ncells, 1), 2), dtype=torch.int64, device=dev)
        tot = torch.zeros(3, dtype=torch.int64, device=dev)
        self.ctx.digest_refine_device(self._view(), self.cols, self.max_keys, filter, bits, bset, sub_bits, cells2,
                                      ncells, tot)
        return cells2[:ncells], ncells >> sub_bits

    def reconcile_refined(self, peer_cells2, bits, bucket_set, sub_bits, filter=None):
        """What this store holds in the second-level cells where its digest_refined differs from a
        peer's: refine, cell diff and refined select over the view with n = max_keys, and one
        encode_device with the arena as the heap (shaped like reconcile). peer_cells2: the peer's
        digest_refined(bits, bucket_set, sub_bits, filter)[0], a tensor or a numpy array of
        (n_set << sub_bits) * 2 64-bit words; bucket_set: a tensor or a numpy array of words, the same
        set on both hubs (see digest_refined for the exchange). Returns (wire bytes, differing cells):
        the rows in store order as change frames, for the peer to decode and merge, and the increasing
        cell numbers (numpy int64) in which the two second levels differ."""
        import torch
        bset = self._set_tensor(bucket_set)
        mine, n_set = self.digest_refined(bits, bset, sub_bits, filter)
        ncells = n_set << sub_bits
        peer = self._set_tensor(peer_cells2)
        if peer.numel() != 2 * ncells:
            raise ValueError(f"peer_cells2 holds {peer.numel()} words, {ncells} cells are {2 * ncells}")
        if ncells == 0:
            return b"", np.zeros(0, np.int64)
        cset = self._zeros((ncells + 63) // 64, torch.int64)
        cnt = self._zeros(2, torch.int64)  # [0] differing cells, [1] rows selected
        self.ctx.digest_diff_cells_device(mine, peer, ncells, cset, cnt[0:1])
        rows = self._out_rows(self.max_keys)
        self.ctx.select_refined_device(self._view(), self.cols, self.max_keys, filter, bits, bset, sub_bits, cset, rows,
                                       None, cnt[1:2])
        return self._encode_rows(rows, cnt[1:2]), self._set_bits(cset)


class Comm:
    """An RCCL communicator owned by libdrp (drp_comm_*): one rank per process."""

    def __init__(self, ctx, comm_id, nranks, rank):
        self.L = lib()
        h = P()
        _chk("drp_comm_init_rank", self.L.drp_comm_init_rank(ctx.h, comm_id, nranks, rank, C.byref(h)))
        self.h, self.nranks, self.rank = h, nranks, rank

    @staticmethod
    def new_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _chk("drp_comm_id", lib().drp_comm_id(buf))
        return buf.raw

    def allgather_index(self, ctx, local_t, global_t, base_t):
        """drp_index_allgather over torch CUDA tensors (int64 (per_rank, 4) local stats)."""
        ctx.order_after_torch(local_t)
        _chk("drp_index_allgather", self.L.drp_index_allgather(ctx.h, self.h, _tp(local_t), local_t.shape[0],
                                                               _tp(global_t), _tp(base_t)))

    def close(self):
        if self.h:
            self.L.drp_comm_destroy(self.h)
            self.h = None
