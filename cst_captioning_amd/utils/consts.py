"""Read-only constant device tensors of the per-step code (the BOS token
vector of a free-running decode, the all-zero seed pair of a dropout-free
FeatPool, ...), made once per (device, shape) instead of by a fill launch in
every step.

Nothing may write into a tensor returned here.  A constant first asked for
while a HIP graph is being captured is NOT cached: it would live in the
graph's private memory pool and be filled by a captured node only.
"""
import torch

_CACHE = {}


def const_tensor(kind, shape, value, dtype, device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        return torch.full(shape, value, dtype=dtype, device=dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (kind, tuple(shape), value, dtype, idx)
    t = _CACHE.get(key)
    if t is None:
        t = torch.full(shape, value, dtype=dtype, device=dev)
        if torch.cuda.is_current_stream_capturing():
            return t
        # (once: any stream may read it afterwards without an event)
        torch.cuda.current_stream(dev).synchronize()
        _CACHE[key] = t
    return t
