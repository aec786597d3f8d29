// drp_order.h — what drp_order.hip (order by `change`) and drp_keyorder.hip (order by key) share: the
// sort workgroup's shape, the small device helpers, the scratch layout, and the launchers of the
// pieces both chains are made of. The digit pass (ord_hist / ord_blocksum / ord_scanbase /
// ord_scatter) and the gather exist once, in drp_order.hip.
#pragma once
#include "drp_device.h"
#include "drp_kernels.h"

namespace drp {

constexpr uint32_t ORD_BLK = 1024, ORD_WAVES = ORD_BLK / 64, ORD_RPL = 4;
constexpr uint32_t ORD_CHUNKS = ORD_TILE / 64, ORD_BINS = 256;
static_assert(ORD_BLK * ORD_RPL == ORD_TILE, "four pairs per lane");

__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
#pragma unroll
  for (uint32_t m = 1; m < WAVE; m <<= 1) {
    const uint32_t lo = shfl_xor32((uint32_t)v, m), hi = shfl_xor32((uint32_t)(v >> 32), m);
    v |= ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// the OR and the AND of a workgroup of ORD_BLK threads' values, in thread 0 (wo, wa: ORD_WAVES words
// of LDS each; every thread calls)
__device__ __forceinline__ void ord_block_or_and(uint64_t &o, uint64_t &a, uint64_t *wo, uint64_t *wa) {
  o = wave_or64(o);
  a = ~wave_or64(~a);
  if (lane_id() == 0) {
    wo[threadIdx.x >> 6] = o;
    wa[threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t k = 1; k < ORD_WAVES; k++) {
      o |= wo[k];
      a &= wa[k];
    }
  }
}

// the segment of row i (b[0] <= i): the greatest f < nseg with b[f] <= i (b non-decreasing)
__device__ __forceinline__ uint32_t ord_seg(const uint64_t *b, uint32_t nseg, uint64_t i) {
  uint32_t lo = 0, hi = nseg;
  for (uint32_t k = 0; k < 7 && hi - lo > 1; k++) {  // (nseg <= 64: six halvings)
    const uint32_t mid = (lo + hi) >> 1;
    if (b[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the source row at sorted position s (fs: OrdCtl::final_src)
__device__ __forceinline__ uint64_t ord_row_at(const OrderParams &P, uint32_t fs, uint64_t b0, uint64_t s) {
  return fs ? (uint64_t)P.idx[fs - 1][s] : b0 + s;
}

// the scratch of a sort over rows_cap entries, and its pointers into P
struct OrdLayout {
  uint64_t nwg, nscan, ctl, por, pand, key[2], idx[2], hist, bsum, end;
  explicit OrdLayout(uint64_t cap) {
    nwg = cap ? (cap + ORD_TILE - 1) / ORD_TILE : 1;
    nscan = (ORD_BINS * nwg + ORD_SCAN - 1) / ORD_SCAN;
    ctl = 0;
    por = 256;
    pand = por + al(nwg * 8);
    key[0] = pand + al(nwg * 8);
    key[1] = key[0] + al(cap * 8);
    idx[0] = key[1] + al(cap * 8);
    idx[1] = idx[0] + al(cap * 4);
    hist = idx[1] + al(cap * 4);
    bsum = hist + al(ORD_BINS * nwg * 4);
    end = bsum + al(nscan * 4);
  }
  void place(OrderParams &P, void *scratch) const {
    uint8_t *sc = static_cast<uint8_t *>(scratch);
    P.ctl = reinterpret_cast<OrdCtl *>(sc + ctl);
    P.part_or = reinterpret_cast<uint64_t *>(sc + por);
    P.part_and = reinterpret_cast<uint64_t *>(sc + pand);
    for (int k = 0; k < 2; k++) {
      P.key[k] = reinterpret_cast<uint64_t *>(sc + key[k]);
      P.idx[k] = reinterpret_cast<uint32_t *>(sc + idx[k]);
    }
    P.hist = reinterpret_cast<uint32_t *>(sc + hist);
    P.bsum = reinterpret_cast<uint32_t *>(sc + bsum);
  }
};
static_assert(sizeof(OrdCtl) <= 256, "the control block's place in the scratch");

}  // namespace drp

// The pieces of a chain, over a P whose scratch pointers are placed: ord_init (row_base checked, the
// counts into the control block), the four kernels of digit pass p as the control block's act[p] /
// src[p] direct it, and the gather of at most out_max (and at most rows_cap) output rows.
extern "C" {
void drp_launch_order_init(const drp::OrderParams *P, hipStream_t st);
void drp_launch_order_pass(const drp::OrderParams *P, uint32_t p, hipStream_t st);
void drp_launch_order_gather(const drp::OrderParams *P, uint64_t out_max, hipStream_t st);
}
