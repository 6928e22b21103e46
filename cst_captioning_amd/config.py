"""Flag system.

Accepts every flag name of the reference (``/root/reference/opts.py:5-345``) so
Makefile recipes written for the reference keep working, plus the new
MI355X-specific flags (data parallelism, precision, kernel selection,
synthetic data).

Reference quirks kept on purpose:
  * ``--optim*`` flags are accepted; the reference ignores them and always
    uses Adam with default betas (``train.py:492``).  We honour them only when
    ``--honor_optim_flags 1`` is given, so defaults reproduce the reference.
  * ``--train_cached_tokens`` is ``type=str`` with an (odd) int default 30.
"""
import argparse
import sys


def reward_mix_arg(spec):
    """``--reward_mix``: '' (off) or a specification ops/reward_mix.py accepts."""
    if spec == '':
        return spec
    from .ops.reward_mix import parse_reward_mix
    try:
        parse_reward_mix(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return spec


def mbr_mix_arg(spec):
    """``--mbr_mix``: '' (CIDEr-D) or a specification of the ``--reward_mix`` grammar."""
    if spec == '':
        return spec
    from .ops.reward_mix import parse_reward_mix
    try:
        parse_reward_mix(spec, '--mbr_mix')
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return spec


def ema_decay_arg(spec):
    """``--ema_decay``: a float in [0, 1); 0 = no EMA."""
    try:
        d = float(spec)
    except ValueError:
        raise argparse.ArgumentTypeError('not a number: %r' % spec)
    if not 0.0 <= d < 1.0:  # (NaN fails the comparison too)
        raise argparse.ArgumentTypeError('--ema_decay must be in [0, 1), got %r' % spec)
    return d


def label_smoothing_arg(spec):
    """``--label_smoothing``: a finite float in [0, 1); 0 = plain cross-entropy."""
    try:
        e = float(spec)
    except ValueError:
        raise argparse.ArgumentTypeError('not a number: %r' % spec)
    if not 0.0 <= e < 1.0:  # (NaN fails the comparison too)
        raise argparse.ArgumentTypeError('--label_smoothing must be in [0, 1), got %r' % spec)
    return e


def mbr_top_k_arg(spec):
    """``--mbr_top_k``: an integer >= 0; 0 = no truncation."""
    try:
        k = int(spec)
    except ValueError:
        raise argparse.ArgumentTypeError('not an integer: %r' % spec)
    if k < 0:
        raise argparse.ArgumentTypeError('--mbr_top_k must be >= 0, got %r' % spec)
    return k


def ensemble_weight_arg(spec):
    """One of ``--ensemble_weights``: a positive finite float."""
    try:
        w = float(spec)
    except ValueError:
        raise argparse.ArgumentTypeError('not a number: %r' % spec)
    if not (w > 0.0 and w != float('inf')):  # (NaN fails the comparison too)
        raise argparse.ArgumentTypeError('--ensemble_weights must be positive and finite, got %r'
                                         % spec)
    return w


def mbr_top_p_arg(spec):
    """``--mbr_top_p``: a finite float in (0, 1]; 1 = no nucleus cut."""
    try:
        p = float(spec)
    except ValueError:
        raise argparse.ArgumentTypeError('not a number: %r' % spec)
    if not 0.0 < p <= 1.0:  # (NaN fails the comparison too)
        raise argparse.ArgumentTypeError('--mbr_top_p must be in (0, 1], got %r' % spec)
    return p


RL_OBJECTIVES = ('reinforce', 'risk', 'softmax_margin', 'multi_margin')


def _finite_float(spec):
    try:
        x = float(spec)
    except ValueError:
        raise argparse.ArgumentTypeError('not a number: %r' % spec)
    return x if x == x and abs(x) != float('inf') else None


def rl_alpha_arg(spec):
    """``--rl_alpha``: a finite float > 0."""
    a = _finite_float(spec)
    if a is None or not a > 0.0:
        raise argparse.ArgumentTypeError('--rl_alpha must be finite and > 0, got %r' % spec)
    return a


def rl_cost_scale_arg(spec):
    """``--rl_cost_scale``: a finite float >= 0."""
    k = _finite_float(spec)
    if k is None or not k >= 0.0:
        raise argparse.ArgumentTypeError('--rl_cost_scale must be finite and >= 0, got %r' % spec)
    return k


def build_parser():
    p = argparse.ArgumentParser(
        description='MI355X-native consensus/self-critical video captioning trainer')
    add = p.add_argument

    # ---- data (opts.py:8-57) -------------------------------------------------
    for split in ('train', 'val', 'test'):
        add('--%s_label_h5' % split, type=str,
            help='path to the label file (h5, or .npz written by this framework)')
        add('--%s_feat_h5' % split, type=str, nargs='+',
            help='path(s) to the per-modality feature file(s)')
        add('--%s_cocofmt_file' % split, type=str,
            help='gold captions in MSCOCO format for language metrics')
    add('--train_bcmrscores_pkl', type=str,
        help='precomputed consensus scores of the GT captions (pkl or npz)')

    # ---- optimisation (opts.py:58-150) --------------------------------------
    add('--max_patience', type=int, default=5)
    add('--batch_size', type=int, default=128)
    add('--test_batch_size', type=int, default=32)
    add('--train_seq_per_img', type=int, default=20)
    add('--test_seq_per_img', type=int, default=20)
    add('--learning_rate', type=float, default=1e-4)
    add('--lr_update', type=int, default=50)
    add('--rnn_type', type=str, default='lstm', choices=['lstm', 'gru', 'rnn'])
    add('--rnn_size', type=int, default=512)
    add('--num_lm_layer', type=int, default=1, help='unused (as in the reference)')
    add('--input_encoding_size', type=int, default=512)
    add('--max_epochs', type=int, default=sys.maxsize)
    add('--grad_clip', type=float, default=0.25)
    add('--drop_prob_lm', type=float, default=0.5)
    add('--optim', type=str, default='adam')
    add('--optim_alpha', type=float, default=0.8)
    add('--optim_beta', type=float, default=0.999)
    add('--optim_epsilon', type=float, default=1e-8)

    # ---- evaluation / checkpointing (opts.py:153-233) -----------------------
    add('--save_checkpoint_from', type=int, default=20)
    add('--save_checkpoint_every', type=int, default=1)
    add('--use_rl', type=int, default=0)
    add('--use_rl_after', type=int, default=30)
    add('--train_cached_tokens', type=str, default=30,
        help='path to the index document-frequency pickle for CIDEr-D')
    add('--expand_feat', type=int, default=1)
    add('--model_file', type=str)
    add('--result_file', type=str)
    add('--start_from', type=str, default='')
    add('--language_eval', type=int, default=1)
    add('--eval_metric', default='CIDEr',
        choices=['Loss', 'Bleu_4', 'METEOR', 'ROUGE_L', 'CIDEr', 'MSRVTT'])
    add('--test_language_eval', type=int, default=1, help='unused (as in the reference)')
    add('--print_log_interval', type=int, default=20)
    add('--loglevel', type=str, default='DEBUG',
        choices=['DEBUG', 'INFO', 'WARNING', 'ERROR', 'CRITICAL'])

    # ---- misc / model (opts.py:234-345) -------------------------------------
    add('--seed', type=int, default=123)
    add('--gpuid', type=int, default=7, help='unused; device comes from LOCAL_RANK')
    add('--num_chunks', type=int, default=1,
        help='1: no attention, > 1: temporal attention over num_chunks frames')
    add('--num_layers', type=int, default=1)
    add('--model_type', type=str, default='concat',
        choices=['standard', 'concat', 'manet'])
    add('--beam_size', type=int, default=5)
    add('--use_ss', type=int, default=0)
    add('--use_ss_after', type=int, default=0)
    add('--ss_max_prob', type=float, default=0.25)
    add('--ss_k', type=float, default=30.0)
    add('--use_mixer', type=int, default=1)
    add('--mixer_from', type=int, default=-1)
    add('--mixer_descrease_every', type=int, default=2)
    add('--use_cst', type=int, default=0)
    add('--use_cst_after', type=int, default=0)
    add('--cst_increase_every', type=int, default=5)
    add('--scb_baseline', type=int, default=1)
    add('--scb_captions', type=int, default=20)
    add('--use_eos', type=int, default=0)
    add('--output_logp', type=int, default=0)

    # ---- new: MI355X framework flags ----------------------------------------
    add('--impl', type=str, default='auto', choices=['auto', 'hip', 'torch'],
        help='decoder implementation: fused HIP engine, or plain PyTorch ops')
    add('--precision', type=str, default='bf16', choices=['bf16', 'fp32'],
        help='decoder compute precision: bf16 = fused HIP engine (bf16 MFMA operands, fp32 '
             'accumulation / master weights); fp32 = PyTorch path in fp32')
    add('--reward_device', type=str, default='gpu', choices=['gpu', 'cpu'],
        help='CIDEr-D reward: on-GPU HIP kernel, or the CPU scorer (reference semantics)')
    add('--reward_mix', type=reward_mix_arg, default='', metavar='METRIC:WEIGHT[,...]',
        help='RL reward = weighted sum of sentence metrics, e.g. CIDEr:1,Bleu_4:5,ROUGE_L:5 '
             '(CIDEr = CIDEr-D on its x10 scale, Bleu_4, ROUGE_L; non-negative weights, a metric '
             'left out has weight 0; METEOR is host-only and cannot be mixed), scored in one '
             'launch on the GPU (ops/reward_mix.py).  --eval_metric then selects the model on '
             'validation only.  Empty (default): the reward is the metric of --eval_metric')
    add('--val_scorer', type=str, default='strings', choices=['strings', 'tokens'],
        help='validation / test metrics: strings = decoded sentences through the Python '
             'scorers (reference route); tokens = token ids against the split\'s label table, '
             'on the GPU when the model runs there (ops/corpus_metrics.py)')
    add('--decode', type=str, default='standard', choices=['standard', 'mbr'],
        help='validation / test decoding: standard = greedy (--beam_size 1) or beam search; '
             'mbr = consensus (minimum-Bayes-risk) decoding: the standard caption plus '
             '--mbr_samples multinomial samples per video, every one scored against the others '
             'under CIDEr-D (ops/mbr.py, on the GPU when the model runs there), the one that '
             'agrees most returned.  Needs a CIDEr-D document-frequency table: the training '
             "set's, or --train_cached_tokens for the test command")
    add('--mbr_samples', type=int, default=20,
        help='--decode mbr: multinomial samples per video beside the standard caption')
    add('--mbr_temperature', type=float, default=1.0,
        help='--decode mbr: sampling temperature of those samples')
    add('--mbr_top_k', type=mbr_top_k_arg, default=0, metavar='K',
        help='--decode mbr: draw each word of those samples from the K most probable words '
             'only (truncated sampling; the temperature applies inside them).  On the fused '
             'engine K <= 8 runs in csrc/kernels/topk_sample.hip, larger K through the PyTorch '
             'path.  0 (default): no truncation')
    add('--mbr_top_p', type=mbr_top_p_arg, default=1.0, metavar='P',
        help='--decode mbr: nucleus inside the --mbr_top_k words: the shortest prefix of them '
             '(most probable first) whose renormalised mass reaches P, in (0, 1]; P < 1 needs '
             '--mbr_top_k >= 1.  1 (default): all K words')
    add('--ensemble_files', type=str, nargs='+', default=[], metavar='FILE',
        help='test: further checkpoints decoded together with --model_file (member 0), at most '
             '8 members in all: every step averages the members\' word probabilities '
             '(models/ensemble.py; csrc/kernels/ensemble.hip on the fused engine).  Each member '
             'is built from its own checkpoint\'s options; vocab, seq_length, feat_dims and '
             'num_chunks must agree.  Not with --decode mbr')
    add('--ensemble_weights', type=ensemble_weight_arg, nargs='+', default=[], metavar='W',
        help='--ensemble_files: one positive weight per member, --model_file first (normalised '
             'to sum 1).  Default: uniform')
    add('--mbr_mix', type=mbr_mix_arg, default='', metavar='METRIC:WEIGHT[,...]',
        help='--decode mbr: the utility the captions of a pool are scored under, in the grammar '
             'of --reward_mix, e.g. CIDEr:1,Bleu_4:5,ROUGE_L:5 (peer CIDEr-D on its x10 scale, '
             'sentence Bleu_4 and ROUGE_L with the other captions of the pool as references), '
             'one launch on the GPU (ops/mbr.py PeerMix).  The document-frequency table is '
             'needed only when CIDEr has a weight.  Empty (default): CIDEr-D')
    add('--consensus_scorer', type=str, default='file', choices=['file', 'tokens'],
        help='GT consensus scores of CST / WXE training: file = read --train_bcmrscores_pkl '
             '(prepro/evalscores.py); tokens = computed at start-up (when --use_cst 1) from the training label '
             'table in the metric of --eval_metric, leave-one-out, on the GPU when the model '
             'runs there (ops/consensus.py); --train_bcmrscores_pkl must then not be given')
    add('--mask_after_eos', type=int, default=0,
        help='fix for SURVEY §2.8.1: mask MIXER tokens sampled after EOS (0 = reference parity)')
    add('--dedupe_greedy', type=int, default=1,
        help='SCST: decode the greedy baseline once per video instead of x seq_per_img '
             '(bit-identical rows; see models/caption_model.py)')
    add('--honor_optim_flags', type=int, default=0,
        help='use --optim_alpha/--optim_beta/--optim_epsilon for Adam (reference ignores them)')
    add('--synthetic', type=str, default='',
        help="'msrvtt' or 'msvd': generate a synthetic dataset of that shape instead of files")
    add('--synthetic_vocab', type=int, default=10509)
    add('--synthetic_videos', type=int, default=0, help='0 = dataset default')
    add('--feat_dims', type=int, nargs='+', default=None,
        help='synthetic feature dims (default: resnet 2048, c3d 4096, mfcc 1024, category 300)')
    add('--seq_length', type=int, default=30, help='synthetic label length')
    add('--save_last', type=int, default=1,
        help='write a _last.pth sidecar with optimizer/RNG/loader state for exact resume')
    add('--nan_guard', type=int, default=1, help='skip a step whose loss is not finite')
    add('--cuda_graph', type=int, default=1,
        help='replay the fused-engine training step as a captured HIP graph (1) or enqueue '
             'it eagerly every step (0)')
    add('--grad_wire', type=str, default='fp32', choices=['fp32', 'bf16'],
        help='data-parallel gradient reduction: fp32 all-reduce, or bf16 on the wire with '
             'fp32 accumulation (all-to-all + all-gather, half the bytes)')
    add('--comm_priority', type=str, default='normal', choices=['high', 'normal'],
        help='data parallelism: priority of the stream that all-reduces the gradient slices '
             'under the backward.  normal (default); high: a hardware queue of its own, '
             'measured to slow the whole replayed step from 3.38 to 5.75 ms '
             '(scripts/dp_standin.py, profiles/r6/dp_standin_rccl.json)')
    add('--dp_update', type=str, default='allreduce', choices=['allreduce', 'sharded'],
        help='data-parallel update: all-reduce the fp32 gradient and run Adam on the whole '
             'buffer on every rank (default), or reduce-scatter -> Adam on this rank\'s '
             '1/N shard (fp32 moments kept for the shard only) -> all-gather the parameters')
    add('--ema_decay', type=ema_decay_arg, default=0.0, metavar='D',
        help='keep an exponential moving average of the parameters, e += (1 - D) (p - e) in '
             'the fused Adam pass, and validate / select / save the best checkpoint with it '
             '(the _last.pth sidecar keeps the live weights, the EMA in its optimizer state).  '
             '0 (default): off')
    add('--label_smoothing', type=label_smoothing_arg, default=0.0, metavar='E',
        help='label smoothing of the XE training loss (XE epochs, also those before '
             '--use_rl_after): per token -[(1 - E) log p(y) + E mean_v log p(v)], the definition '
             'of torch cross_entropy(label_smoothing=E); on the fused engine its uniform part '
             'rides the exp-store backward as rank-1 terms (no dense log-probs).  RL / WXE '
             'losses, the validation loss and every decode ignore it.  0 (default): off')
    add('--rl_objective', type=str, default='reinforce', choices=list(RL_OBJECTIVES),
        help='RL objective: reinforce (default) = REINFORCE with the baseline of the recipe '
             '(SCST / CST); risk, softmax_margin, multi_margin = sequence-level structured losses '
             'over each video\'s --train_seq_per_img sampled captions (expected risk; '
             'softmax-margin and multi-margin against the best-scored sample), on their '
             'length-normalised log-probabilities and the scores of the reward scorer '
             '(models/criteria.py GroupCriterion; one launch on the fused path, '
             'ops/scst_loss.py group_loss).  No greedy decode; --scb_captions / --scb_baseline '
             'are ignored.  Needs --use_rl 1 --use_mixer 1 --expand_feat 1 and at least 2 '
             'captions per video')
    add('--rl_alpha', type=rl_alpha_arg, default=1.0, metavar='A',
        help='--rl_objective risk / *_margin: scale of the length-normalised sequence scores '
             '(finite, > 0)')
    add('--rl_cost_scale', type=rl_cost_scale_arg, default=1.0, metavar='K',
        help='--rl_objective risk / *_margin: cost of a caption = K * (best score of the '
             'video\'s samples - its score) (finite, >= 0)')
    add('--profile_phases', type=int, default=0, help='log per-phase HIP-event timings')
    return p


def parse_opts(argv=None):
    p = build_parser()
    opt = p.parse_args(argv)
    if opt.mbr_top_p < 1.0 and opt.mbr_top_k == 0:
        p.error('--mbr_top_p < 1 needs --mbr_top_k >= 1 (the nucleus is taken inside the '
                'top-k candidates)')
    if opt.ensemble_weights and not opt.ensemble_files:
        p.error('--ensemble_weights needs --ensemble_files')
    return opt


def default_opts(**overrides):
    """Namespace with every default, optionally overridden (used by tests/bench)."""
    opt = build_parser().parse_args([])
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt
