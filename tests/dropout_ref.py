"""Restatement of the fused tuning step's train-mode dropout (DESIGN.md §19;
models.py:300,311,354), for the tests: the Philox4x32-10 masks from their
definition in numpy, and the fp64 / fp32 torch forward with the five
multiplications inserted.  Shared by test_dropout_ref.py (CPU) and
test_gpu_dropout.py.

Masks: for element e of dropout site s in optimizer step n under a 64-bit
seed, key = (seed_lo, seed_hi), counter = (e >> 2, s, n_lo, n_hi), the word is
output word e & 3; dropped iff word < (uint32)(p * 2^32), the product in
double with p the fp32 value the C-ABI receives.  Kept elements are scaled by
1 / (1 - p) in fp32.
"""
import math

import numpy as np
import torch

from oracle import pregan_train_oracle as TO

T = torch
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
# the mask cases of the GPU test: seeds (one below 2^32, one above) and (base, launch step) pairs
# for optimizer steps 0, 1 and 2^32 + 5; test_dropout_ref.py holds their drop counts within 5 sigma
TEST_SEEDS = (7, (3 << 32) | 12345)
TEST_STEPS = ((0, 0), (0, 1), (1 << 32, 5))


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (uint32 values) -> [..., 4] uint32 words; ten
    rounds, the key bumped by (W0, W1) after each."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & m32, p1 & m32,
             ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & m32, p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return np.stack(c, axis=-1).astype(np.uint32)


def site_counts(H):
    """Elements per site, in site order 0..8."""
    layer = [18 * H, 3 * H * H, 192 * H, 3 * H * H]
    return [3 * H * H] + layer + layer


def drop_threshold(p):
    return int(float(np.float32(p)) * 4294967296.0)


def keep_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_masks(H, p, seed, step):
    """One step's keep bytes (1 = kept) in site order, uint8 [sum(site_counts)]."""
    thr = drop_threshold(p)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    key = np.array([seed & MASK32, seed >> 32], dtype=np.uint64)
    out = []
    for s, n in enumerate(site_counts(H)):
        e = np.arange(n, dtype=np.uint64)
        ctr = np.stack([e >> np.uint64(2), np.full(n, s, np.uint64), np.full(n, step & MASK32, np.uint64),
                        np.full(n, step >> 32, np.uint64)], axis=-1)
        words = philox4x32_10(ctr, np.broadcast_to(key, (n, 2)))
        word = words[np.arange(n), (e & np.uint64(3)).astype(np.int64)]
        out.append((word.astype(np.uint64) >= np.uint64(thr)).astype(np.uint8))
    return np.concatenate(out)


def split_masks(keep, H, dtype=T.float64):
    """Keep bytes in site order -> the tensors encode_drop_t multiplies by:
    pe / d1{l} / d2{l} [1,3,H,H], ff{l} [1,3,H,64] (token t = w*H + h), attn{l}
    [1,H,2,3,3]: the canonical [3(w), H, 2(head), 3(key step)] permuted to
    encode_t's [b, n=H, head, s, t]."""
    keep = np.asarray(keep)
    cnt = site_counts(H)
    assert keep.size == sum(cnt)
    parts = np.split(keep.astype(np.float64), np.cumsum(cnt)[:-1])
    tt = lambda a: T.tensor(np.ascontiguousarray(a), dtype=dtype)
    m = {"pe": tt(parts[0].reshape(1, 3, H, H))}
    for l in range(2):
        at, d1, ff, d2 = parts[1 + 4 * l:5 + 4 * l]
        m[f"attn{l}"] = tt(at.reshape(3, H, 2, 3).transpose(1, 2, 0, 3)[None])
        m[f"d1{l}"] = tt(d1.reshape(1, 3, H, H))
        m[f"ff{l}"] = tt(ff.reshape(1, 3, H, 64))
        m[f"d2{l}"] = tt(d2.reshape(1, 3, H, H))
    return m


def unit_masks():
    return {k: 1.0 for k in ["pe"] + [f"{s}{l}" for s in ("attn", "d1", "ff", "d2") for l in (0, 1)]}


def _lin(x, w, b):
    return x @ w.T + b


def encode_drop_t(tw, win, m, scale):
    """oracle.pregan_train_oracle.encode_t with the five dropout
    multiplications (mask * scale) inserted: win [B,W,3H] -> latent [B,3H^2]."""
    B, Wn, F = win.shape
    H = F // 3
    x = win.reshape(B, Wn, H, 3)
    fc, at = tw["gat.layer1.heads.0.fc.weight"], tw["gat.layer1.heads.0.attn_fc.weight"]
    z = x @ fc.T
    d = fc.shape[0]
    s = z @ at[0, :d]
    t = z @ at[0, d:]
    e = s[..., :, None] + t[..., None, :]
    e = T.nn.functional.leaky_relu(e, 0.01)
    a = T.softmax(e.reshape(B, Wn, H * H), dim=-1).reshape(B, Wn, H, H)
    g = T.einsum("bwij,bwid->bwjd", a, z)
    h = _lin(g, tw["time_encoder.weight"], tw["time_encoder.bias"])
    h = (h + tw["pos_encoder.pe"][:Wn].reshape(1, Wn, 1, -1)) * m["pe"] * scale
    for li in range(2):
        p = f"transformer_encoder.layers.{li}."
        hd = d // 2
        qkv = _lin(h, tw[p + "self_attn.in_proj_weight"], tw[p + "self_attn.in_proj_bias"])
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        q = q.reshape(B, Wn, H, 2, hd)
        k = k.reshape(B, Wn, H, 2, hd)
        v = v.reshape(B, Wn, H, 2, hd)
        sc = T.einsum("bsnhe,btnhe->bnhst", q, k) / math.sqrt(hd)
        pr = T.softmax(sc, dim=-1) * m[f"attn{li}"] * scale
        o = T.einsum("bnhst,btnhe->bsnhe", pr, v).reshape(B, Wn, H, d)
        sa = _lin(o, tw[p + "self_attn.out_proj.weight"], tw[p + "self_attn.out_proj.bias"]) * m[f"d1{li}"] * scale
        h = T.nn.functional.layer_norm(h + sa, (d,), tw[p + "norm1.weight"], tw[p + "norm1.bias"], 1e-5)
        f1 = T.relu(_lin(h, tw[p + "linear1.weight"], tw[p + "linear1.bias"])) * m[f"ff{li}"] * scale
        ff = _lin(f1, tw[p + "linear2.weight"], tw[p + "linear2.bias"]) * m[f"d2{li}"] * scale
        h = T.nn.functional.layer_norm(h + ff, (d,), tw[p + "norm2.weight"], tw[p + "norm2.bias"], 1e-5)
    return h.permute(0, 2, 1, 3).reshape(B, -1)


def autograd_drop(w, x, y, mult, tgt, m, scale, dtype=T.float64):
    """The step's loss (CE * mult + the positive prototype MSE, as
    test_gpu_train._autograd) through encode_drop_t + decode_t, backward run:
    returns (leaf params with .grad, logits [B,H,2], protos [B,H,2])."""
    B, H = y.shape
    tw = TO.leaf_params(w["transformer"], dtype=dtype)
    lat = encode_drop_t(tw, T.tensor(np.asarray(x), dtype=dtype), m, scale)
    logits, protos = TO.decode_t(tw, lat)
    ce = T.nn.functional.cross_entropy(logits.reshape(-1, 2), T.tensor(np.asarray(y).reshape(-1), dtype=T.long),
                                       reduction="none").reshape(B, H)
    loss = (ce * T.tensor(np.asarray(mult), dtype=dtype)).sum()
    mse = ((protos - T.tensor(np.asarray(tgt), dtype=dtype)) ** 2).mean(-1)
    loss = loss + (mse * T.tensor(np.asarray(y) > 0)).sum()
    loss.backward()
    return tw, logits.detach().double().numpy(), protos.detach().double().numpy()


def spiky_case(H, seed):
    """Inputs as test_gpu_train._batched_case makes them at B = 1: synthetic
    weights (seed 3 there), a window with spikes, labels, CE weights and
    prototype targets."""
    rng = np.random.Generator(np.random.PCG64(9 + H + 1 + 1000 * seed))
    x = rng.uniform(0, 0.8, size=(1, 3, 3 * H))
    spike = rng.uniform(size=x.shape) < 0.03
    x = np.where(spike, rng.uniform(0.9, 1.3, size=x.shape), x)
    y = (rng.uniform(size=(1, H)) < 0.3).astype(np.int32)
    mult = rng.uniform(0.5, 2.0, size=(1, H))
    tgt = rng.uniform(0, 1, size=(1, H, 2))
    return x, y, mult, tgt


def ratio_to_tolerance(got, want, rel, abs_scale):
    """max |got - want| / (rel * |want| + abs_scale * max|want|): <= 1 passes
    the project's `close`."""
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    tol = rel * np.abs(want) + abs_scale * (np.abs(want).max() + 1e-30)
    return float((np.abs(got - want) / tol).max())


def drop_key_bias(name, a, d):
    """Without the attention key-bias slice (identically-zero gradient:
    rounding noise on both sides, test_gpu_train.key_bias_mask)."""
    a = np.asarray(a).reshape(-1)
    if name.endswith("self_attn.in_proj_bias"):
        return np.concatenate([a[:d], a[2 * d:]])
    return a
