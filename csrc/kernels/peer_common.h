// Limits and the n-gram list of a pool row, shared by the peer kernels of
// consensus (MBR) decoding: cider_pairwise.hip and peer_mix.hip.
#pragma once
#include "../common.h"

namespace cst {

constexpr int PEER_MAXT = 63;          // compact_hypothesis: one wave, W <= 63 (+ EOS)
constexpr int PEER_MAXG = 64;
constexpr int PEER_MAX_SLOTS = 2048;   // G * (T + 1): 64 x 32 or 32 x 64
constexpr int PEER_HDR_BYTES = 32;
constexpr int PEER_WAVES = 16;

// The n-grams of a row of W tokens as one list: order n + 1 has max(W - n, 0)
// entries and starts at o[n]; o[4] is the total.
struct PeerSpan {
  int o1, o2, o3, E;
  __device__ __forceinline__ explicit PeerSpan(int W) {
    o1 = W;
    o2 = o1 + max(W - 1, 0);
    o3 = o2 + max(W - 2, 0);
    E = o3 + max(W - 3, 0);
  }
  // entry x -> order index n (0..3) and position in the order
  __device__ __forceinline__ int order(int x, int& pos) const {
    const int n = (x >= o1) + (x >= o2) + (x >= o3);
    pos = x - (n == 0 ? 0 : n == 1 ? o1 : n == 2 ? o2 : o3);
    return n;
  }
};

}  // namespace cst
