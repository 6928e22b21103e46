// Sentence-level BLEU-4 / ROUGE-L rewards: per-dataset reference tables and
// the native CPU scorers (see metric_host.cpp).
#pragma once
#include <stdint.h>

#include <vector>

namespace cst {

constexpr int METRIC_MAXT = 64;            // hypothesis width and reference length limit
constexpr int64_t METRIC_MAX_TOKEN = 65534;  // BLEU: token + 1 must fit the 16-bit packing

struct MetricTables {
  std::vector<int32_t> vid_ref_off;  // (Nv + 1) references of video v: [off[v], off[v+1])
  std::vector<int32_t> ref_len;      // (nref) reduced length of every reference
  // BLEU: per video the union of its references' n-grams (n <= 4) as packed
  // keys in ascending order (which groups them by order), each with the
  // maximum count over the references (the clip count)
  std::vector<int32_t> vid_ng_off;   // (Nv + 1)
  std::vector<int64_t> ng_key;
  std::vector<int32_t> ng_cnt;
  // leave-one-out BLEU: the in-video index of the reference that alone attains
  // ng_cnt (-1 when several do), and the largest count among the other
  // references (0 when no other has the n-gram)
  std::vector<int32_t> ng_cnt2;
  std::vector<int32_t> ng_arg;
  // ROUGE: the reduced reference token rows, ragged
  std::vector<int32_t> ref_tok_off;  // (nref + 1)
  std::vector<int32_t> ref_tok;
  // METEOR (validation scorer): the stem id of every ref_tok entry; filled
  // only when the builder is given the vocabulary's stem ids
  std::vector<int32_t> ref_stem;
};

struct MetricTablesView {
  int Nv;
  const int32_t* vid_ref_off;
  const int32_t* ref_len;
  const int32_t* vid_ng_off;
  const int64_t* ng_key;
  const int32_t* ng_cnt;
  const int32_t* ref_tok_off;
  const int32_t* ref_tok;
  // (leave-one-out BLEU only; a view without them scores without exclusion)
  const int32_t* ng_cnt2 = nullptr;
  const int32_t* ng_arg = nullptr;
};

inline MetricTablesView view_of(const MetricTables& t) {
  return {(int)t.vid_ref_off.size() - 1, t.vid_ref_off.data(), t.ref_len.data(),
          t.vid_ng_off.data(),           t.ng_key.data(),      t.ng_cnt.data(),
          t.ref_tok_off.data(),          t.ref_tok.data(),     t.ng_cnt2.data(),
          t.ng_arg.data()};
}

// Throws std::invalid_argument when a reference is longer than METRIC_MAXT
// tokens or holds a token outside [0, METRIC_MAX_TOKEN].
// stem_ids (V entries, optional): also fills ref_stem; a reference token >= V
// is then rejected too.
MetricTables build_metric_tables(const int64_t* labels, int M, int L, const int64_t* start,
                                 const int64_t* end, int Nv, int use_eos,
                                 const int32_t* stem_ids = nullptr, int V = 0);

// (N, T) hypotheses, T <= METRIC_MAXT (std::invalid_argument otherwise; BLEU
// also rejects tokens above METRIC_MAX_TOKEN).  A video without references
// scores 0.
// exclude (N, optional): leave-one-out scoring, exclude[i] = the in-video index
// of a reference that hypothesis i does not see (excluded_ref, cider_common.h:
// ignored when negative, past the video's references, or the only reference).
// BLEU needs a view with ng_cnt2 / ng_arg for it (std::invalid_argument).
void bleu4_score_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                      const MetricTablesView& t, int use_eos, float* out,
                      const int64_t* exclude = nullptr);
void rouge_l_score_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                        const MetricTablesView& t, int use_eos, float* out,
                        const int64_t* exclude = nullptr);

// Peer scoring under a mixed utility (peer_mix_host.cpp; consensus / MBR decoding,
// the twin of csrc/kernels/peer_mix.hip): hyps (N, T) in pools of G consecutive rows, the
// references of row i are the G - 1 other rows of its pool.  parts (N, 3) = peer
// CIDEr-D (cider_peers_host), sentence BLEU-4 and ROUGE-L against those
// references -- i.e. build_metric_tables on the pool rows + the scorers above with
// exclude[i] = i mod G; out (N) = ((w[0] * c) + (w[1] * b)) + (w[2] * r) in fp32.
// A metric of weight 0 is not computed and its column is exactly 0; the df hash
// table is read only when w[0] != 0 and may be null otherwise.  Any G >= 2 with
// N % G == 0, T <= METRIC_MAXT, finite non-negative weights that are not all
// zero (std::invalid_argument otherwise; CIDEr-D and BLEU also reject tokens
// above METRIC_MAX_TOKEN).
void peer_mix_host(const int64_t* hyps, int N, int T, int G, const int64_t* ht_keys,
                   const float* ht_vals, uint32_t ht_cap, double log_ref_len, int use_eos,
                   const double w[3], float* out, float* parts);

// Validation scorer (ops/corpus_metrics.py), fp64 host twins of
// csrc/kernels/corpus_metrics.hip.  Hypotheses are reduced without EOS.
//  * bleu_stats_host: per hypothesis correct[4], guess[4], tlen, rlen (10 ints),
//    the summands of Bleu.compute_score's corpus value;
//  * meteor_stats_host: Meteor._align / _stats of the best reference by
//    Meteor._score (the first on ties): n_exact, n_stem, len_h, len_r, chunks,
//    n_pairs (6 ints) and the segment score.  ref_stem is the table's stem row,
//    stem_ids the V stem ids of the vocabulary.
void bleu_stats_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                     const MetricTablesView& t, int32_t* out);
void meteor_stats_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                       const MetricTablesView& t, const int32_t* ref_stem,
                       const int32_t* stem_ids, int V, int32_t* out_stats, double* out_score,
                       const int64_t* exclude = nullptr);
double meteor_score_host(int n_exact, int n_stem, int len_h, int len_r, int chunks);

}  // namespace cst
