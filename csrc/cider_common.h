// CIDEr-D shared definitions (host + device).
//
// An n-gram (n <= 4) of token ids is packed exactly into 64 bits: token t of
// position i occupies bits [16i, 16i+16) as t + 1, so 0 is "unused" and the
// key is collision-free for vocabularies up to 65534 ids (same packing as
// cst_captioning_amd/prepro/ciderdf.py:pack_ngram).
//
// The document-frequency table is an open-addressing hash table with linear
// probing: keys[cap] (0 = empty), vals[cap], cap a power of two.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CST_HD __host__ __device__ __forceinline__
#else
#define CST_HD inline
#endif

namespace cst {

CST_HD uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

CST_HD int ngram_order(uint64_t key) {
  return 1 + ((key >> 16) != 0) + ((key >> 32) != 0) + ((key >> 48) != 0);
}

// df lookup; 0 when absent (the upstream scorer's defaultdict(float))
CST_HD float df_lookup(const int64_t* keys, const float* vals, uint32_t cap, uint64_t key) {
  uint32_t h = (uint32_t)mix64(key) & (cap - 1);
  for (uint32_t probe = 0; probe < cap; ++probe) {
    uint64_t k = (uint64_t)keys[h];
    if (k == key) return vals[h];
    if (k == 0) return 0.f;
    h = (h + 1) & (cap - 1);
  }
  return 0.f;
}

// Leave-one-out scoring (GT consensus scores): exclude[hyp] = e leaves out
// reference e of the hypothesis' video, counted from the start of the video's
// range [r0, r1) of vid_ref_off.  Returns the absolute index of the reference to
// skip, or -1 for none: a null array, e < 0, e >= the number of references, or a
// video with a single reference (which is then kept:
// prepro/evalscores.py `rest if rest else refs[v]`).
CST_HD int excluded_ref(const int64_t* exclude, int hyp, int r0, int r1) {
  if (!exclude) return -1;
  const int64_t e = exclude[hyp];
  return (e >= 0 && e < (int64_t)(r1 - r0) && r1 - r0 > 1) ? r0 + (int)e : -1;
}

#if defined(__HIPCC__)
// Hypothesis compaction shared by the reward kernels (cider_d.hip,
// sent_metrics.hip), run by ONE whole wavefront on row `row` of (., T <= 64)
// tokens: reproduces array_to_str -- drop BOS (=1) anywhere, stop at the first
// EOS (=0) and keep that 0 when use_eos.  Writes the W kept tokens to
// s_tok[0..W) (64 ints, LDS) and returns W (<= 64), the same in every lane.
// The caller orders the LDS writes before other lanes' reads.
__device__ __forceinline__ int compact_hypothesis(const int64_t* __restrict__ row, int T, int lane,
                                                  int use_eos, int* s_tok) {
  const int tok = lane < T ? (int)row[lane] : 0;
  const uint64_t zmask = __ballot(lane >= T || tok == 0);
  const int e = zmask ? __ffsll((long long)zmask) - 1 : 64;  // first EOS (or end)
  const bool keep = lane < e && tok != 1;
  const uint64_t kmask = __ballot(keep);
  const int pos = __popcll(kmask & ((1ull << lane) - 1ull));
  int W = __popcll(kmask);
  if (keep) s_tok[pos] = tok;
  if (use_eos && e < T) {
    if (lane == 0) s_tok[W] = 0;
    W += 1;
  }
  return W;
}
#endif

}  // namespace cst
