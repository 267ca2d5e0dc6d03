"""The host side of every AdamW step here: which tensors step, their counts, and
the per-step scalars each kernel reads as a descriptor or a table row,

    active,  step_size = lr / (1 - b1^step),  bc2_sqrt = sqrt(1 - b2^step).

The only place in the package that forms a bias correction.  The arithmetic is
torch's single-tensor AdamW's (torch/optim/adamw.py): Python floats,
``beta ** step`` and ``math.sqrt``, rounded to fp32 once; numpy's vectorised
``**`` gives other doubles at some steps.  numpy and ctypes only:
no torch, no device."""
from __future__ import annotations

import math

import numpy as np

from ._native import _AdamTensor

COND_TENSORS = ("prototype_decoder.0.weight", "prototype_decoder.0.bias")   # no gradient without a positive label


def scalars(lr, b1, b2, steps):
    """(step_size, bc2_sqrt) of the step counts ``steps``, fp32 arrays of its
    shape: one Python-float evaluation per distinct count.  A tensor that has
    never stepped (count 0) gets the scalars of step 1."""
    steps = np.maximum(np.asarray(steps, dtype=np.float64), 1.0)
    lo = np.floor(steps.min()) if steps.size else 1.0
    off = (steps - lo).astype(np.int64)
    if off.max(initial=0) <= 4 * off.size + 64 and (off + lo == steps).all():
        # whole counts in a narrow range, as a run's are: the distinct ones without a sort
        seen = np.bincount(off.ravel()) > 0
        uniq, inv = np.flatnonzero(seen) + lo, (np.cumsum(seen) - 1)[off]
    else:
        uniq, inv = np.unique(steps, return_inverse=True)
        inv = inv.reshape(steps.shape)
    size = np.array([lr / (1 - b1 ** s) for s in uniq.tolist()], dtype=np.float32)
    bc2 = np.array([math.sqrt(1 - b2 ** s) for s in uniq.tolist()], dtype=np.float32)
    return size[inv], bc2[inv]


def schedule(steps0, on, lr, b1, b2):
    """The tables of n consecutive steps: steps0 [..., T] the tensors' counts
    (fp64) before them, on [..., n, T] whether tensor k steps at step s (torch
    skips a parameter without a gradient) -> (table [..., n, T, 3] fp32 of
    (on, step_size, bc2_sqrt), the counts [..., T] after them).  A skipped
    tensor's row repeats the scalars of its last step; one that has never
    stepped gets those of step 1.  Pure: the caller stores the counts back."""
    steps0, on = np.asarray(steps0, dtype=np.float64), np.asarray(on, dtype=bool)
    steps = steps0[..., None, :] + np.cumsum(on, axis=-2)
    table = np.empty(on.shape + (3,), dtype=np.float32)
    table[..., 0] = on
    table[..., 1], table[..., 2] = scalars(lr, b1, b2, steps)
    return table, steps0 + on.sum(axis=-2)


def stepping(names, positive, cond_names=COND_TENSORS):
    """``schedule``'s ``on`` [..., n, T] for the tuning pattern: the tensors
    named in cond_names step only at the steps with positive[..., n]."""
    cond = np.array([name in cond_names for name in names], dtype=bool)
    return np.where(cond, np.asarray(positive, dtype=bool)[..., None], True)


def descriptors(tensors, rows=None):
    """The ctypes ``pgp_adam_tensor`` array of the tensors' (offset, n), with
    ``rows`` [T, 3] = (active, step_size, bc2_sqrt) for a launch that reads
    them from its descriptors; without, (1, 0, 0): a table-driven launch reads
    only the places."""
    if rows is None:
        rows = ((1, 0.0, 0.0),) * len(tensors)
    return (_AdamTensor * len(tensors))(*[_AdamTensor(t["offset"], t["n"], int(a), float(s), float(b))
                                          for t, (a, s, b) in zip(tensors, rows)])
