// Entry points of the native extension that bindings.cpp binds: the one place
// they are declared.  Each is defined in the unit named above its group.
#pragma once
#include <torch/extension.h>

#include <map>
#include <string>
#include <vector>

namespace cst {

// decoder_forward.cpp / decoder_backward.cpp / beam_search.cpp
std::vector<at::Tensor> decoder_forward(at::Tensor wx, at::Tensor emb, at::Tensor ptab,
                                        at::Tensor whh, at::Tensor wlog,
                                        at::Tensor blog, at::Tensor vgate, int64_t vgate_div,
                                        at::Tensor labels, at::Tensor bos, int64_t R, int64_t T,
                                        std::vector<int64_t> modes, double ss_prob,
                                        double drop_p, double temperature, at::Tensor rng,
                                        bool save, bool want_xe, bool use_counts,
                                        bool use_unfinished, std::vector<at::Tensor> att,
                                        int64_t cell, std::vector<at::Tensor> state0,
                                        std::vector<at::Tensor> up, bool store_exp,
                                        bool xe_rows, c10::optional<at::Tensor> lab_idx,
                                        double ls_eps, c10::optional<at::Tensor> ls_wbar);
std::vector<at::Tensor> decoder_backward(at::Tensor wx, at::Tensor wlog, at::Tensor emb,
                                         at::Tensor lse, at::Tensor logits16,
                                         at::Tensor hdrop_all, at::Tensor gates_all,
                                         at::Tensor c_all, at::Tensor h_all, at::Tensor seq,
                                         at::Tensor labels, at::Tensor toks, at::Tensor dg_sel,
                                         at::Tensor dg_xe, double drop_p, at::Tensor rng,
                                         at::Tensor out_wlog, at::Tensor out_blog,
                                         int64_t comm_stream, std::vector<at::Tensor> att,
                                         at::Tensor out_emb, at::Tensor ds_bias, int64_t cell,
                                         std::vector<at::Tensor> state0,
                                         std::vector<at::Tensor> up, at::Tensor blog,
                                         at::Tensor fix_total, int64_t vgate_div,
                                         at::Tensor xw, std::vector<at::Tensor> vg_bwd,
                                         int64_t vg_nf, double vg_p, int64_t x_wait,
                                         bool exp_zero_off, std::vector<at::Tensor> dw_slots,
                                         c10::optional<at::Tensor> vg_idx, int64_t vg_C,
                                         double ls_eps, c10::optional<at::Tensor> ls_wbar);
std::vector<at::Tensor> beam_search(at::Tensor wx, at::Tensor ptab, at::Tensor whh,
                                    at::Tensor wlog, at::Tensor blog, at::Tensor vgate,
                                    int64_t K, int64_t T, int64_t bos_index,
                                    std::vector<at::Tensor> att, int64_t cell,
                                    std::vector<at::Tensor> state0, std::vector<at::Tensor> up,
                                    int64_t rows_per_video = 0, double top_p = 1.0,
                                    double temperature = 1.0,
                                    c10::optional<at::Tensor> rng = c10::nullopt,
                                    std::vector<std::vector<at::Tensor>> ensemble = {},
                                    std::vector<double> ens_weights = {},
                                    bool ens_greedy = false);

// engine.cpp: the executor's shared state
void set_stamp_base(int64_t base);
void stamp_buffer(at::Tensor buf);
void stamp_now(int64_t slot);
int64_t wall_clock_khz();
void set_grad_events(bool on);
void grad_event_wait(int64_t k, int64_t stream);
void grad_event_record(int64_t k, int64_t stream);
int64_t grad_event_count(int64_t k);
void set_poll_bound(int64_t n);
void set_bwd_loop(int64_t mode);
void set_att_fuse(bool on);
int64_t device_errors(int64_t dev_index);
void reset_device_errors(int64_t dev_index);
void vocab_x(at::Tensor logits16, at::Tensor wlog, at::Tensor out);

// host/blaslt_tuned.cpp
void gemm_bf16_tuned(at::Tensor out, at::Tensor a, bool ta, at::Tensor b, bool tb,
                     int64_t n_cand);
void gemm_bf16_tuned_batched(at::Tensor out, at::Tensor a, bool ta, at::Tensor b, bool tb,
                             int64_t n_cand);
std::vector<double> gemm_tuned_timings(at::Tensor out, at::Tensor a, bool ta, at::Tensor b,
                                       bool tb);
std::vector<std::vector<double>> gemm_tuned_choices();

// train_ops.cpp
at::Tensor featpool_forward(std::vector<at::Tensor> xs, std::vector<at::Tensor> ws,
                            std::vector<at::Tensor> bs, double drop_p, at::Tensor rng,
                            c10::optional<at::Tensor> idx, int64_t C);
std::vector<at::Tensor> featpool_forward16(std::vector<at::Tensor> xs, std::vector<at::Tensor> ws,
                                           std::vector<at::Tensor> bs, double drop_p,
                                           at::Tensor rng, c10::optional<at::Tensor> idx,
                                           int64_t C);
std::vector<at::Tensor> featpool_backward(at::Tensor dout, at::Tensor out,
                                          std::vector<at::Tensor> xs,
                                          std::vector<at::Tensor> ws, double drop_p,
                                          std::vector<at::Tensor> outs,
                                          c10::optional<at::Tensor> idx, int64_t C);
std::vector<at::Tensor> cst_loss_forward(at::Tensor seq, at::Tensor lp, at::Tensor scores,
                                         at::Tensor bref, int64_t S, int64_t k, int64_t objective,
                                         double alpha, double cost_scale);
std::vector<at::Tensor> scst_loss_forward(at::Tensor seq, at::Tensor lp, at::Tensor sample,
                                          at::Tensor greedy);
std::vector<at::Tensor> xe_loss_forward(at::Tensor labels, at::Tensor lp, int64_t off);
at::Tensor xe_loss_backward(at::Tensor cnt, at::Tensor out, at::Tensor dloss, int64_t T);
at::Tensor scst_loss_backward(at::Tensor seq, at::Tensor reward, at::Tensor out,
                              at::Tensor dloss, c10::optional<at::Tensor> row_weight);
at::Tensor cider_score(at::Tensor hyps, at::Tensor hyp_video, std::map<std::string, at::Tensor> t,
                       double log_ref_len, int64_t use_eos, bool clipped,
                       c10::optional<at::Tensor> exclude, int64_t group);
at::Tensor bleu_stats(at::Tensor hyps, at::Tensor hyp_video, std::map<std::string, at::Tensor> t);
std::vector<at::Tensor> meteor_stats(at::Tensor hyps, at::Tensor hyp_video,
                                     std::map<std::string, at::Tensor> t, at::Tensor stem_ids,
                                     c10::optional<at::Tensor> exclude);
at::Tensor metric_score(const std::string& metric, at::Tensor hyps, at::Tensor hyp_video,
                        std::map<std::string, at::Tensor> t, int64_t use_eos,
                        c10::optional<at::Tensor> exclude);
std::vector<at::Tensor> reward_mix_score(
    at::Tensor hyps, at::Tensor hyp_video,
    c10::optional<std::map<std::string, at::Tensor>> cider_tables,
    c10::optional<std::map<std::string, at::Tensor>> sent_tables, double log_ref_len,
    int64_t use_eos, std::vector<double> weights);
std::vector<at::Tensor> peer_mix_score(at::Tensor hyps,
                                       c10::optional<std::map<std::string, at::Tensor>> df,
                                       double log_ref_len, int64_t use_eos,
                                       std::vector<double> weights, int64_t group);
at::Tensor flat_adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                          at::Tensor partials, at::Tensor scal, at::Tensor skip, at::Tensor hyper,
                          double b1, double b2, double eps, double clip, double gscale,
                          int64_t phase, at::Tensor shadow_meta,
                          std::vector<at::Tensor> shadow_dst, c10::optional<at::Tensor> ema,
                          double ema_decay);
void refresh_shadows(at::Tensor p, at::Tensor shadow_meta, std::vector<at::Tensor> shadow_dst,
                     c10::optional<at::Tensor> swap_with);

// dev_entries.cpp: test and microbenchmark entries
double lstm_bwd_loop_bench(int64_t R, int64_t H, int64_t T, int64_t iters, at::Tensor phases,
                           int64_t dbg);
std::vector<at::Tensor> lstm_step_bwd_test(
    at::Tensor dg_next, at::Tensor whhT, at::Tensor dh_logit, at::Tensor dc_carry,
    at::Tensor gates, at::Tensor c_t, at::Tensor c_prev, double drop_p, at::Tensor rng,
    int64_t step, int64_t cell, int64_t KD, int64_t sentinel,
    c10::optional<at::Tensor> dh_scale, c10::optional<at::Tensor> oh_W,
    c10::optional<at::Tensor> oh_a, c10::optional<at::Tensor> oh_ys,
    c10::optional<at::Tensor> oh_b, c10::optional<at::Tensor> oh_yx,
    c10::optional<at::Tensor> gvb16, int64_t vdiv, int64_t C);
std::vector<at::Tensor> lstm_bwd_loop_test(
    at::Tensor whhT, at::Tensor dh, at::Tensor gates, at::Tensor c_all, double drop_p,
    at::Tensor rng, int64_t cell, int64_t form, c10::optional<at::Tensor> scale,
    c10::optional<at::Tensor> oh_W, c10::optional<at::Tensor> oh_a,
    c10::optional<at::Tensor> oh_ys, c10::optional<at::Tensor> oh_b,
    c10::optional<at::Tensor> oh_yx);
double vocab_fwd_bench(at::Tensor hd, at::Tensor wlog, at::Tensor blog, at::Tensor tgt,
                       int64_t flags, bool save, int64_t iters, int64_t variant);
double vgrad_colsum_bench(at::Tensor E, at::Tensor alpha, int64_t V, int64_t iters);
double token_sort_bench(at::Tensor toks, int64_t V, int64_t iters);
double att_bench(at::Tensor gv, at::Tensor P, at::Tensor q, at::Tensor wa, at::Tensor ba,
                 int64_t R, int64_t which, int64_t iters);
at::Tensor att_mfma_phases(at::Tensor gv, at::Tensor P, at::Tensor wa, at::Tensor ba, int64_t R);
std::vector<at::Tensor> att_mfma_fwd(at::Tensor h, at::Tensor wq, at::Tensor P, at::Tensor wa,
                                     at::Tensor ba, at::Tensor gv,
                                     int64_t whole);
std::vector<at::Tensor> vocab_select(at::Tensor hd, at::Tensor wlog, at::Tensor blog,
                                     at::Tensor rng, int64_t mode, double temperature,
                                     int64_t step, int64_t top_k = 0, double top_p = 1.0);
// kernels/ensemble.hip alone (tests; the ens_* mode of the vocab_select binding)
std::vector<at::Tensor> ensemble_topk_test(std::vector<at::Tensor> logits,
                                           std::vector<at::Tensor> lse, std::vector<double> logw,
                                           int64_t V, int64_t K,
                                           c10::optional<at::Tensor> unfinished,
                                           bool baseline = false);
std::vector<at::Tensor> decode_step_test(at::Tensor hd, at::Tensor h, at::Tensor wlog,
                                         at::Tensor blog, at::Tensor whh, at::Tensor vgate,
                                         int64_t vdiv, at::Tensor tgt, at::Tensor eoff,
                                         int64_t save, int64_t mode, int64_t step, at::Tensor rng,
                                         at::Tensor ptab, at::Tensor c_prev, double drop_p,
                                         int64_t cell, int64_t eos, at::Tensor unfinished,
                                         double ss_prob, bool want_xe = true);
std::vector<at::Tensor> token_sort(at::Tensor toks, int64_t V);
at::Tensor token_group_sum(at::Tensor x, at::Tensor toks, int64_t V);
std::vector<at::Tensor> vgrad_fold(at::Tensor E, at::Tensor lse, at::Tensor y_sel,
                                   at::Tensor dg_sel, at::Tensor labels, at::Tensor dg_xe,
                                   int64_t V, int64_t zero_off, at::Tensor hd, at::Tensor wlog,
                                   at::Tensor blog, at::Tensor fix_total, bool forward_x,
                                   at::Tensor X, double ls_eps,
                                   c10::optional<at::Tensor> ls_wbar);
at::Tensor vgrad_rows(at::Tensor alpha, at::Tensor hd, int64_t ldhs, at::Tensor dhd);
at::Tensor vgrad_colsum(at::Tensor E, at::Tensor alpha, int64_t V, int64_t ls_mode, double ls_eps,
                        c10::optional<at::Tensor> ls_dg, c10::optional<at::Tensor> ls_dw,
                        c10::optional<at::Tensor> ls_db);
at::Tensor video_gate_grad(at::Tensor dG, int64_t vdiv, int64_t G4);
at::Tensor wgrad_tn(at::Tensor A, at::Tensor B, int64_t M, int64_t N, int64_t K);
void wgrad_tn_rows(at::Tensor A, at::Tensor B, int64_t M, int64_t N, int64_t K, at::Tensor out,
                   at::Tensor rmap);
std::vector<at::Tensor> wgrad_tn_colsum(at::Tensor A, at::Tensor B, at::Tensor al, int64_t M,
                                        int64_t N, int64_t K);
void busy_copy(at::Tensor buf, int64_t blocks, double us, int64_t stream);

}  // namespace cst
