// drp_ctx.h — the device context behind the C ABI (struct drp_ctx of include/drp.h) and the small
// host helpers its translation units share (drp_api.hip: decode, fetch, encode, life cycle;
// drp_relay.hip: select, latest per key, fan-out).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../include/drp.h"
#include "drp_kernels.h"  // (al)

namespace drp {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool ensure(size_t n) {
    if (n <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 4 + 4096;
    if (hipMalloc(&p, want) != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();  // (the failure is reported by the caller, not by a later launch)
      return false;
    }
    cap = want;
    return true;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *at(size_t off) const {
    return reinterpret_cast<T *>(static_cast<char *>(p) + off);
  }
};

// Page-locked host memory that only grows (the gather buffer of chunked host batches).
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool ensure(size_t n) {
    if (n <= cap) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 4 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return false;
    }
    cap = want;
    return true;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

inline bool is_device_ptr(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// page-locked host memory (the DMA engine reads it directly, without a staging copy)
inline bool is_pinned_host(const void *p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

}  // namespace drp

struct drp_ctx {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {};
  hipEvent_t hev[2] = {};  // a staged piece's H2D
  // pipelined staging (stage_pieces): the copy stream and one event per chunk (created on first use)
  hipStream_t cst = nullptr;
  hipEvent_t pev[32] = {};
  // their early fetches: a fetch stream, the event behind a piece's last row writes, and a pinned
  // bounce buffer the rows land in before a worker thread copies them into the caller's columns
  hipStream_t fst = nullptr;
  hipEvent_t fev = nullptr;
  drp::PinBuf fbounce;
  uint64_t pipe_chunk = 128ull << 20;  // DRP_PIPE_CHUNK (MiB; 0: no pipelining)
  uint32_t B = 128;
  int strict = 0;
  int exact = 0;  // 1: always the exact kernel (decode_tiles), never the speculative one
  int key_post = 0;  // DRP_KEY_POST_*: key hashes and/or key flags on every decode
  // claims_fast's structural check of long frames: on after a decode whose frames average
  // >= 512 bytes (or none yet); DRP_CHANGE_CHECKS=0/1 forces it (A/B, tests)
  int change_checks = 1, change_checks_env = -1;
  int cus = 256;
  uint32_t waves_per_cu = 16;
  // test / measurement knobs, read once by drp_open (never on a decode): DRP_KSTRONG_HBM weakens
  // predictions, DRP_DIRTY_CAP caps the repair dirty lists, DRP_STATS / DRP_TRACE_FILE collect
  // kernel counters and per-tile traces into dstats (allocated here when asked for)
  uint32_t kstrong_hbm = 0;
  uint32_t cascade_min = 4096;  // DRP_CASCADE_MIN (tests: small cascades)
  int64_t jump_min = -1;        // DRP_JUMP_MIN (-1: max(64, tiles / 512))
  // claims kernel: the region walkers (drp_walk.hip) for batches of at least walk_min tiles,
  // claims_fast below; DRP_CLAIMS=walk / fast forces one (A/B, tests)
  uint64_t walk_min = 32768;
  int claims_mode = 0;  // 0 auto, 2 fast, 3 hop
  int crec = 1;         // claims_fast's per-frame records and the record emission (DRP_CREC=0: off)
  drp::DevBuf recbuf;
  uint64_t dirty_cap = ~0ull;
  bool stats = false;
  const char *trace_file = nullptr;
  unsigned long long *dstats = nullptr;
  uint32_t *ctile = nullptr;  // segmented repair: per-tile candidate positions (grown on demand)
  uint64_t ctile_cap = 0;
  drp::DevBuf scratch, in_stage, out_stage, aux;
  drp::PinBuf gather;  // chunked host batches: the staged ranges, gathered (drp_decode_stage_v)
  drp::DevBuf dec_cols;  // device columns of the staged host-batch decode (drp_decode_stage)
  drp::DevBuf fetch_tmp; // drp_decode_fetch_block: the caller's block layout, packed on the device
  drp::DevBuf keybuf;    // drp_decode_fetch_keys: per-row key lengths and positions
  drp::DevBuf keytext;   // drp_decode_fetch_keys: the key text
  double frames_per_byte = 0;  // density of the last staged batch (sizes the next one's columns)
  int blob_skip = DRP_BLOB_SKIP_AUTO;
  uint64_t latest_hash_mask = ~0ull;  // drp_set_latest_hash_mask (test hook)
  uint32_t fanout_latest_pass = 0;    // drp_set_fanout_latest_pass (test hook; 0: FLAT_PASS_DEFAULT)
  int order_skip = 1;                 // drp_order_device switches constant-digit passes off (DRP_ORDER_SKIP=0: A/B)
  bool blob_heavy = false;     // the last host batch was mostly blob payload (AUTO: stage in pieces)
  uint64_t blob_run = 0;       // bytes from a piece's start to its blob's payload, last seen
  uint64_t piece_span = 0;     // batch bytes one blob-skipping piece covered on average, last seen
  drp_timing timing = {};
  std::vector<uint64_t> host_tmp;
  // fan-out: the filter table on its way to the device (page-locked; fan_ev: the copy of the last
  // call has left it), and drp_fanout_staged's selected rows and splice ranks
  drp::PinBuf fan_tab;
  hipEvent_t fan_ev = nullptr;
  drp::DevBuf fan_rows;
  // drp_store_merge_news_staged's news column (one byte per delivered GPU row) for
  // drp_fanout_news_staged, and the staged batch (staged.seq) it belongs to
  drp::DevBuf news;
  bool news_held = false;
  uint64_t news_seq = 0;
  // drp_store_lookup_staged's lack_type column (one byte per store row) for its select
  drp::DevBuf lack;
  // the staged host-batch decode: row 0 is a host-built blob continuation when nf0 == 1; GPU
  // rows follow, each piece's payload_off relative to the batch offset where that piece was
  // staged (pieces: {first GPU row, batch offset}; one piece unless blobs were skipped)
  struct Staged {
    uint64_t rows = 0, nf0 = 0, cap = 0;
    std::vector<std::pair<uint64_t, uint64_t>> pieces;
    const uint8_t *dev = nullptr;  // the last piece's bytes on the device (a one-piece batch: all of it)
    // drp_relay_staged: the batch's bytes from batch offset `base` on as they lie on the device
    // (every piece at its own batch offset, the skipped blob payloads as holes), the delivered GPU
    // rows (no malformed Change), and whether a staged batch is held at all
    const uint8_t *wire = nullptr;
    uint64_t wire_bytes = 0, base = 0, good = 0;
    bool valid = false;
    uint64_t seq = 0;  // counts the stage calls: what was derived from an earlier batch is told apart
    struct Row0 {  // the continuation's row (nf0 == 1)
      uint64_t off = 0;
      uint32_t len = 0;
      uint8_t type = 0;
    } row0;
    drp_frames fr = {};
    drp_changes co = {};
  } staged;
};

#define CHK(x)                                                                     \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      if (getenv("DRP_DEBUG")) fprintf(stderr, "drp: %s -> %s\n", #x, hipGetErrorString(e_)); \
      return DRP_E_HIP;                                                            \
    }                                                                              \
  } while (0)
