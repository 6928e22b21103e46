"""HBM-resident dataset and batch loader.

Reference: ``/root/reference/dataloader.py:15-218`` reads h5 features video by
video in a Python loop every batch.  Here the whole split (MSR-VTT train:
~6.5k videos x ~7.5k floats = ~0.2 GB) is uploaded to device memory once;
a batch is an index gather on the GPU.  Per-batch host work is only the
caption-slot choice (numpy, B x S ints) and one small H2D index copy.

Batch semantics kept from the reference:
  * ``seq_per_img`` captions per video: all captions plus uniform random
    repeats when ``ncap <= S``, otherwise the first ``S`` of a random
    permutation (``dataloader.py:125-135``);
  * masks cover the caption plus its EOS (``nonzeros + 1``, ``:158-163``);
  * ``gts`` = every GT label row of the video (for the reward);
  * the epoch counter advances when the iterator wraps, and the train order
    is reshuffled every epoch (``:146-152``).

Data parallelism: all ranks share the shuffle seed, so they see the same
global order; rank ``r`` takes videos ``[r*B, (r+1)*B)`` of each global batch
of ``world_size * B`` videos (weak scaling; ``world_size=1`` is the reference).
"""
import logging

import numpy as np
import torch

from . import formats

logger = logging.getLogger(__name__)


class VideoCaptionDataset:
    """One split: vocabulary, labels, per-modality features, optional
    consensus scores, GT references and the CIDEr-D df table."""

    def __init__(self, vocab, videos, feats, labels=None, label_start_ix=None,
                 label_end_ix=None, bcmrscores=None, gt_refs=None, cocofmt_file=None,
                 df=None):
        self.vocab = list(vocab)
        self.ix_to_word = {i: w for i, w in enumerate(self.vocab)}
        self.videos = [str(v) for v in videos]
        self.video_ids = np.array([int(v) for v in self.videos], dtype=np.int64)
        self.feats = [np.asarray(f, dtype=np.float32) for f in feats]
        for f in self.feats:
            if f.ndim != 3 or f.shape[0] != len(self.videos):
                raise ValueError('features must be (N, C, dim), got %s' % (f.shape,))
        self.labels = None if labels is None else np.asarray(labels, dtype=np.int64)
        self.label_start_ix = None if labels is None else np.asarray(label_start_ix, np.int64)
        self.label_end_ix = None if labels is None else np.asarray(label_end_ix, np.int64)
        if self.labels is not None:
            ncap = self.label_end_ix - self.label_start_ix
            if (ncap <= 0).any():
                raise ValueError('No captions!!')
        self.bcmrscores = None if bcmrscores is None else np.asarray(bcmrscores, np.float64)
        self.gt_refs = gt_refs
        self.cocofmt_file = cocofmt_file
        self.df = df  # (keys uint64, values float32, ref_len)
        self._device_cache = {}

    # -- reference getters (dataloader.py:172-218) ---------------------------
    @property
    def has_label(self):
        return self.labels is not None

    @property
    def num_videos(self):
        return len(self.videos)

    @property
    def seq_length(self):
        return self.labels.shape[1]

    @property
    def vocab_size(self):
        return len(self.vocab)

    @property
    def feat_dims(self):
        return [f.shape[2] for f in self.feats]

    @property
    def num_chunks(self):
        return self.feats[0].shape[1]

    def gts_of(self, vid_index):
        return self.labels[self.label_start_ix[vid_index]:self.label_end_ix[vid_index]]

    def refs(self):
        """GT references {video_id: [captions]} for language evaluation."""
        if self.gt_refs is None and self.cocofmt_file:
            from ..eval import load_gt_refs
            self.gt_refs = load_gt_refs(self.cocofmt_file)
        return self.gt_refs

    def device_tensors(self, device):
        """Features/labels uploaded once and cached per device."""
        key = str(device)
        if key not in self._device_cache:
            fs = [torch.from_numpy(f) for f in self.feats]
            if (len(fs) > 1 and all(f.shape[:-1] == fs[0].shape[:-1] and f.dtype == fs[0].dtype
                                    and f.shape[-1] % 4 == 0 for f in fs)):
                # one (N, [C,] sum d) array, the modalities as column views: a batch
                # is ONE row gather (FeatPool reads column slices with 16-byte
                # aligned rows) instead of one gather launch per modality
                cat = torch.cat(fs, -1).to(device)
                offs = [0]
                for f in fs:
                    offs.append(offs[-1] + f.shape[-1])
                d = {'feats': [cat[..., offs[i]:offs[i + 1]] for i in range(len(fs))],
                     'feats_cat': (cat, offs)}
            else:
                d = {'feats': [f.to(device) for f in fs]}
            if self.has_label:
                d['labels'] = torch.from_numpy(self.labels).to(device)
            if self.bcmrscores is not None:
                d['bcmrscores'] = torch.from_numpy(self.bcmrscores).float().to(device)
            self._device_cache[key] = d
        return self._device_cache[key]

    @classmethod
    def from_files(cls, label_file, feat_files, num_chunks=1, bcmrscores_file=None,
                   eval_metric='CIDEr', cocofmt_file=None, df_file=None):
        store = formats.load_label_file(label_file)
        feats = [formats.load_feature_file(p, store['videos'], num_chunks) for p in feat_files]
        bcmr = None
        if bcmrscores_file:
            from ..prepro.evalscores import load_scores
            bcmr = load_scores(bcmrscores_file, eval_metric)
        df = None
        if df_file and isinstance(df_file, str):
            from ..prepro.ciderdf import load_packed_df
            df = load_packed_df(df_file)
        return cls(store['vocab'], store['videos'], feats, store.get('labels'),
                   store.get('label_start_ix'), store.get('label_end_ix'), bcmr,
                   cocofmt_file=cocofmt_file, df=df)


class CaptionLoader:
    """Batch iterator over a :class:`VideoCaptionDataset` (reference
    ``DataLoader`` API: ``get_batch``, ``reset``, getters, epoch counter)."""

    def __init__(self, dataset, batch_size, seq_per_img, mode='train', device='cpu',
                 rank=0, world_size=1, seed=123):
        self.ds = dataset
        self.batch_size = batch_size
        self.seq_per_img = seq_per_img
        self.mode = mode
        self.device = torch.device(device)
        self.rank = rank
        self.world_size = world_size
        self.iterator = 0
        self.epoch = 0
        self.index = np.arange(dataset.num_videos)
        self._order_rng = np.random.RandomState(seed)          # shared by all ranks
        self._cap_rng = np.random.RandomState(seed * 1009 + 7 + rank)  # rank-local
        if mode == 'train':
            self.shuffle_videos()

    # -- reference getters ----------------------------------------------------
    def get_vocab(self):
        return self.ds.ix_to_word

    def get_vocab_size(self):
        return self.ds.vocab_size

    def get_feat_dims(self):
        return self.ds.feat_dims

    def get_seq_length(self):
        return self.ds.seq_length

    def get_seq_per_img(self):
        return self.seq_per_img

    def get_num_videos(self):
        return self.ds.num_videos

    def get_batch_size(self):
        return self.batch_size

    def get_current_epoch(self):
        return self.epoch

    def set_current_epoch(self, epoch):
        self.epoch = epoch

    def get_current_index(self):
        return self.iterator

    def set_current_index(self, index):
        self.iterator = index

    def reset(self):
        self.iterator = 0

    def shuffle_videos(self):
        self._order_rng.shuffle(self.index)

    @property
    def has_label(self):
        return self.ds.has_label

    @property
    def cocofmt_file(self):
        return self.ds.cocofmt_file

    def state_dict(self):
        return {'iterator': self.iterator, 'epoch': self.epoch, 'index': self.index.copy(),
                'order_rng': self._order_rng.get_state(), 'cap_rng': self._cap_rng.get_state()}

    def load_state_dict(self, s):
        self.iterator, self.epoch = s['iterator'], s['epoch']
        self.index = np.asarray(s['index'])
        self._order_rng.set_state(s['order_rng'])
        self._cap_rng.set_state(s['cap_rng'])

    # -- batching ---------------------------------------------------------------
    def _next_videos(self):
        """Dataset indices of this rank's videos for the next batch."""
        n = self.ds.num_videos
        take = []
        for g in range(self.batch_size * self.world_size):
            idx = self.index[self.iterator]
            if self.rank * self.batch_size <= g < (self.rank + 1) * self.batch_size:
                take.append(idx)
            self.iterator += 1
            if self.iterator >= n:
                logger.info('===> Finished loading epoch %d', self.epoch)
                self.iterator = 0
                self.epoch += 1
                if self.mode == 'train':
                    self.shuffle_videos()
        return np.array(take, dtype=np.int64)

    def _caption_rows(self, vids):
        """``seq_per_img`` label rows per video (dataloader.py:119-131): all
        captions in order plus uniform random repeats when ncap <= S, a
        uniformly random subset in random order when ncap > S.  Vectorised
        over the batch (the per-video Python loop cost ~0.5 ms per step)."""
        S = self.seq_per_img
        st = self.ds.label_start_ix[vids].astype(np.int64)
        ncap = self.ds.label_end_ix[vids].astype(np.int64) - st
        j = np.arange(S, dtype=np.int64)[None, :]
        pick = np.broadcast_to(j, (len(vids), S)).copy()
        short = ncap < S
        if short.any():
            nc = ncap[short][:, None]
            rep = (self._cap_rng.random_sample((int(short.sum()), S)) * nc).astype(np.int64)
            pick[short] = np.where(j < nc, j, np.minimum(rep, nc - 1))
        long_ = ncap > S
        if long_.any():
            nc = ncap[long_][:, None]
            keys = self._cap_rng.random_sample((int(long_.sum()), int(nc.max())))
            keys[np.arange(keys.shape[1])[None, :] >= nc] = np.inf
            pick[long_] = np.argsort(keys, axis=1)[:, :S]
        return (st[:, None] + pick).reshape(-1)

    def _to_device(self, *arrays):
        """int64 host arrays -> device tensors through one pinned staging
        buffer and one asynchronous copy (pageable copies block the host)."""
        if self.device.type != 'cuda':
            return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
        sizes = [len(a) for a in arrays]
        n = sum(sizes)
        if getattr(self, '_pin', None) is None or self._pin.numel() < n:
            self._pin = torch.empty(max(n, 1 << 16), dtype=torch.int64).pin_memory()
            self._pin_event = None
        if self._pin_event is not None:
            self._pin_event.synchronize()  # previous copy out of the buffer is done
        host = self._pin.numpy()
        off = 0
        for a, k in zip(arrays, sizes):
            host[off:off + k] = a
            off += k
        tgt = getattr(self, '_index_target', None)
        if tgt is not None and tgt.numel() == n:
            # the captured step's static index buffer: one host->device copy
            # straight into it, stream-ordered after the previous replay that
            # read it (Trainer._graph_step then has nothing to copy)
            dev = tgt
            dev.copy_(self._pin[:n], non_blocking=True)
            self._pin_event = torch.cuda.Event()
            self._pin_event.record()
        else:
            dev = self._pin[:n].to(self.device, non_blocking=True)
            self._pin_event = torch.cuda.Event()
            self._pin_event.record()
        out, off = [], 0
        for k in sizes:
            out.append(dev[off:off + k])
            off += k
        return out

    def set_index_target(self, flat):
        """Upload the index arrays of every later batch whose total length
        equals ``flat.numel()`` into ``flat`` (a graph-captured step's static
        index buffer) instead of a fresh device tensor.  Batches alias it: a
        batch's indices are valid until the next batch is assembled."""
        self._index_target = flat

    def get_batch(self):
        return self._assemble(self._next_videos())

    def get_batch_at(self, ii):
        """Evaluation batch ``ii`` of the fixed order: videos
        ``[ii*B, min((ii+1)*B, N))``.  This equals the reference's
        wrap-around batch followed by the last-batch truncation
        (``train.py:296-308``) and lets ranks take disjoint batches."""
        lo = ii * self.batch_size
        hi = min(lo + self.batch_size, self.ds.num_videos)
        return self._assemble(self.index[lo:hi].astype(np.int64))

    def _assemble(self, vids):
        rows = self._caption_rows(vids) if self.has_label else None
        idx = self._to_device(vids, rows) if rows is not None else self._to_device(vids)
        return Batch(self, vids, idx)

    def feature_tables(self):
        """The HBM-resident feature tables, one (videos, C, d_f) tensor per
        modality (column slices of the concatenated table where there is one):
        what a consumer that reads rows by index takes instead of a gathered
        copy (:class:`IndexedFeats`)."""
        return list(self.ds.device_tensors(self.device)['feats'])

    def gather(self, vid_t, rows_t=None, keys=None):
        """Device part of a batch from its index tensors: features, labels,
        masks (``nonzeros + 1``, ``dataloader.py:158-163``) and consensus
        scores -- gathers only, so it can run inside a captured HIP graph.
        ``keys``: the subset to build (default: all)."""
        dev = self.ds.device_tensors(self.device)
        keys = set(keys) if keys is not None else {'feats', 'labels', 'masks', 'bcmrscores'}
        out = {}
        if 'feats' in keys:
            if 'feats_cat' in dev:
                cat, offs = dev['feats_cat']
                g = cat.index_select(0, vid_t)
                out['feats'] = [g[..., offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
            else:
                out['feats'] = [f.index_select(0, vid_t) for f in dev['feats']]
        if rows_t is not None:
            if keys & {'labels', 'masks'}:
                labels = dev['labels'].index_select(0, rows_t)
                out['labels'] = labels
                if 'masks' in keys:
                    n = (labels != 0).sum(1, keepdim=True) + 1
                    pos = torch.arange(labels.shape[1], device=labels.device)[None, :]
                    out['masks'] = (pos < n).float()
            if 'bcmrscores' in keys:
                out['bcmrscores'] = dev['bcmrscores'].index_select(0, vid_t) \
                    if 'bcmrscores' in dev else None
        return out


class IndexedFeats:
    """A batch's features as (resident tables, video index) for a consumer
    that reads the rows by index (the fused FeatPool: no gathered copy inside
    the step).  For everybody else it is the sequence of gathered (B, C, d_f)
    tensors -- iterating, indexing or :meth:`gathered` makes the batch's one
    gathered copy (``batch['feats']``) on the current stream."""

    def __init__(self, batch, tables, index):
        self._batch = batch
        self.tables = tables  # [(videos, C, d_f)] per modality
        self.index = index    # (B,) int64 rows of the tables

    def gathered(self):
        return self._batch['feats']

    def __len__(self):
        return len(self.tables)

    def __iter__(self):
        return iter(self.gathered())

    def __getitem__(self, i):
        return self.gathered()[i]


class IndexedLabels:
    """A batch's label rows as (resident (captions, L) table, caption-row
    index) for a consumer that reads them by index (the fused decoder's
    rollout: no gathered copy inside the step).  :meth:`gathered` is the
    batch's one gathered copy (``batch['labels']``), made on the current
    stream on first use."""

    def __init__(self, batch, table, index):
        self._batch = batch
        self.table = table  # (captions, L) int64
        self.index = index  # (R,) int64 rows of the table

    def gathered(self):
        return self._batch['labels']

    def size(self, d):
        return self.index.numel() if d == 0 else self.table.size(d)


class LazyGather(dict):
    """The device part of a batch (``feats``, ``labels``, ``masks``,
    ``bcmrscores``), each gathered on its first access: a step that never
    reads the masks (SCST) never launches their kernels, also inside a
    captured graph."""

    _DEVICE_KEYS = ('feats', 'labels', 'masks', 'bcmrscores')

    def __init__(self, loader, idx):
        super().__init__()
        self._loader = loader
        self._idx = idx  # [vid_t] or [vid_t, rows_t]
        self._touched = False

    def _materialise(self, k):
        if not dict.__contains__(self, k):
            self._touched = True
            self.update(self._loader.gather(*self._idx, keys=[k]))
            if not dict.__contains__(self, k):  # no labels in this split
                dict.__setitem__(self, k, None)

    def __getitem__(self, k):
        if k in self._DEVICE_KEYS:
            self._materialise(k)
        return super().__getitem__(k)

    def feats_indexed(self):
        """The features as :class:`IndexedFeats` (tables + this batch's video
        index), without gathering anything; None once ``feats`` was gathered
        (the caller may have modified the copy: use it)."""
        if dict.__contains__(self, 'feats'):
            return None
        f = getattr(self, '_ifeats', None)
        if f is None:
            f = self._ifeats = IndexedFeats(self, self._loader.feature_tables(), self._idx[0])
        return f

    def labels_indexed(self):
        """The labels as :class:`IndexedLabels` (the resident table + this
        batch's caption rows), without gathering anything; None where the
        split has no labels or ``labels`` was already gathered (use the
        copy)."""
        if len(self._idx) < 2 or dict.__contains__(self, 'labels'):
            return None
        lab = getattr(self, '_ilabels', None)
        if lab is None:
            table = self._loader.ds.device_tensors(self._loader.device)['labels']
            lab = self._ilabels = IndexedLabels(self, table, self._idx[1])
        return lab

    def get(self, k, default=None):
        if k in self._DEVICE_KEYS:
            self._materialise(k)
        return super().get(k, default)

    def __contains__(self, k):
        if k in self._DEVICE_KEYS:
            self._materialise(k)
            return super().get(k) is not None
        return super().__contains__(k)


class Batch(LazyGather):
    """One batch: ``video_index`` / ``vids`` / ``ids`` / ``gts`` eagerly, the
    device gathers on first access (:class:`LazyGather`).
    ``index_tensors()`` exposes the gather indices, so the trainer's HIP-graph
    step copies only them and gathers inside the graph."""

    def __init__(self, loader, vids, idx):
        super().__init__(loader, idx)
        self['video_index'] = idx[0]
        self['vids'] = vids
        self['ids'] = loader.ds.video_ids[vids].tolist()
        if loader.has_label:
            self['gts'] = _LazyGts(loader.ds, vids)

    def index_tensors(self):
        """The gather indices, or None once a device part was materialised
        (the caller may have modified it, so only an eager step is exact)."""
        return None if self._touched else list(self._idx)


class _LazyGts:
    """List-like per-video GT label arrays, materialised only if a CPU
    scorer asks for them (the GPU reward never does)."""

    def __init__(self, ds, vids):
        self.ds, self.vids = ds, vids

    def __len__(self):
        return len(self.vids)

    def __getitem__(self, i):
        return self.ds.gts_of(self.vids[i])

    def __iter__(self):
        return (self[i] for i in range(len(self)))
