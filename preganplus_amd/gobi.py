"""GOBI on MI355X — the schedule producer upstream of the decision path.

Replaces the optimiser of ``GOBIScheduler.run_GOBI`` (``scheduler/GOBI.py:19-42``):
``opt()`` (``scheduler/BaGTI/src/opt.py:17-33``) over the ``energy_latency_16``
surrogate (``scheduler/BaGTI/src/models.py:8-27``), batched over independent
environments, one ``pgp_gobi_optimize`` launch (``csrc/pgp_gobi.hip``).  Its
result's allocation columns are ``env.scheduler.result_cache``, the schedule
input of ``PreGANPlusRecovery.run_model`` (``recovery/PreGANPlus.py:117``).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _native

H = 16
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gobi_energy_latency_16.npz")
_ORDER = ("find.0.weight", "find.0.bias", "find.2.weight", "find.2.bias", "find.4.weight", "find.4.bias",
          "find.6.weight", "find.6.bias")


def load_weights(path=_DATA):
    """The surrogate's state dict (fp32) and the dataset's max container IPS
    (scheduler/BaGTI/src/utils.py:61), as packaged from the reference checkpoint
    by tests/golden/make_golden_gobi.py."""
    z = np.load(path)
    return {k: np.asarray(z[k], dtype=np.float32) for k in _ORDER}, float(z["max_ips"])


def _blob(weights) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([np.asarray(weights[k], np.float32).reshape(-1) for k in _ORDER]))


def check_model_of(model_of, n_env, n_models) -> np.ndarray:
    """model_of as the int32 [E] array the planner takes; ValueError for another
    length or an index outside [0, n_models)."""
    mo = np.asarray(model_of)
    if mo.ndim != 1 or mo.shape[0] != n_env or (mo.size and not np.issubdtype(mo.dtype, np.integer)):
        raise ValueError(f"model_of must be {n_env} integers (one per environment), got {mo.dtype} {mo.shape}")
    if mo.size and (mo.min() < 0 or mo.max() >= n_models):
        raise ValueError(f"model_of has an index outside [0, {n_models})")
    return np.ascontiguousarray(mo, dtype=np.int32)


def pack_signs(v) -> np.ndarray:
    """Probes [..., 16, 18] of +-1 -> uint32 [..., 9]: bit k (row-major entry
    k = c * 18 + f) of word k >> 5 set means +1 (pgp_gobi_so_optimize's signs)."""
    v = np.asarray(v)
    bits = (v.reshape(*v.shape[:-2], 9, 32) > 0).astype(np.uint64)
    return (bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_signs(words) -> np.ndarray:
    """uint32 [..., 9] -> float32 [..., 16, 18] of +-1 (pack_signs' inverse)."""
    w = np.asarray(words, dtype=np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return (2.0 * bits.reshape(*w.shape[:-1], H, H + 2) - 1.0).astype(np.float32)


def _philox4x32_10_word0(c0, c1, k0, k1) -> np.ndarray:
    """Output word 0 of Philox4x32-10 (Salmon et al., SC'11; csrc/pgp_philox.hpp)
    for counters (c0, c1, 0, 0) and keys (k0, k1): uint32 arrays, broadcast."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, k0, k1 = (np.asarray(a, dtype=np.uint64) for a in np.broadcast_arrays(c0, c1, k0, k1))
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0.astype(np.uint32)


def _seeds_u64(seeds) -> np.ndarray:
    """Integer seeds (any signedness, Python ints up to 2^64 - 1) as uint64 [E]."""
    if isinstance(seeds, torch.Tensor):
        seeds = seeds.cpu().numpy()
    if isinstance(seeds, np.ndarray) and np.issubdtype(seeds.dtype, np.integer):
        return np.ascontiguousarray(seeds.astype(np.uint64).reshape(-1))
    return np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)


def so_signs(seeds, steps) -> np.ndarray:
    """The probes pgp_gobi_so_optimize generates from seeds [E], as its explicit
    signs: uint32 [E, steps, 9], word w of step s = output word 0 of
    Philox4x32-10 with key seeds[e] (low, high word) and counter (w, s, 0, 0)."""
    s = _seeds_u64(seeds).reshape(-1, 1, 1)
    step = np.arange(int(steps), dtype=np.uint64).reshape(1, -1, 1)
    word = np.arange(9, dtype=np.uint64).reshape(1, 1, -1)
    return _philox4x32_10_word0(word, step, s & np.uint64(0xFFFFFFFF), s >> np.uint64(32))


class GOBIOptimizer:
    """Batched opt(): init [E,16,18] -> (result [E,16,18], iterations [E], fitness [E]).

    weights: one state dict, or a list of them (a fleet whose cells have their
    own surrogates, as the reference's GOBIScheduler.__init__ loads its
    data_type's own, GOBI.py:11-17); ``optimize(init, model_of=...)`` then runs
    each environment against its own."""

    def __init__(self, weights: dict | list | None = None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError("GOBIOptimizer runs on the GPU only (no CPU fallback)")
        self.max_ips = None   # known for the packaged weights alone; a trained surrogate's comes from its dataset
        if weights is None:
            weights, self.max_ips = load_weights()
        L = _native.lib()
        # the fleet entries; a PGP_LIB build from before them (an A/B against an older library) serves one model
        fleet = hasattr(L, "pgp_gobi_create_many")
        self._L = L
        many = isinstance(weights, (list, tuple))
        if many and not weights:
            raise ValueError("an empty list of surrogates")
        if many and not fleet:
            raise _native.NativeError(f"{_native.LIB_PATH} has no pgp_gobi_create_many: a list of surrogates needs it")
        blobs = [_blob(w) for w in (weights if many else [weights])]
        for blob in blobs:
            if blob.size != L.pgp_gobi_weight_len(H):
                raise ValueError(f"GOBI weight blob {blob.size} != {L.pgp_gobi_weight_len(H)}")
        torch.cuda.set_device(self.device)
        vp = ctypes.c_void_p
        h = vp()
        if many:
            blob = np.ascontiguousarray(np.stack(blobs))
            rc = L.pgp_gobi_create_many(H, len(blobs), blob.ctypes.data_as(vp), blob.size, ctypes.byref(h))
        else:
            blob = blobs[0]
            rc = L.pgp_gobi_create(H, blob.ctypes.data_as(vp), blob.size, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(f"pgp_gobi_create: {rc} {L.pgp_gobi_last_error().decode()}")
        self._h = h
        self.n_models = int(L.pgp_gobi_model_count(h)) if fleet else 1
        self._plans = {}   # model_of's bytes -> (device table, groups)

    def set_model(self, m, weights):
        """Replace surrogate m (a cell whose surrogate was retrained).  A
        blocking upload: call it between optimisations, not during one."""
        if not 0 <= int(m) < self.n_models:
            raise IndexError(f"model {m} outside [0, {self.n_models})")
        blob = _blob(weights)
        if blob.size != self._L.pgp_gobi_weight_len(H):
            raise ValueError(f"GOBI weight blob {blob.size} != {self._L.pgp_gobi_weight_len(H)}")
        torch.cuda.set_device(self.device)
        rc = self._L.pgp_gobi_set_model(self._h, int(m), blob.ctypes.data_as(ctypes.c_void_p), blob.size)
        if rc != 0:
            raise RuntimeError(f"pgp_gobi_set_model: {rc} {self._L.pgp_gobi_last_error().decode()}")

    def plan(self, model_of, n_env):
        """The device group table of a model_of [E] (pgp_gobi_plan_groups),
        cached by its content: (int32 tensor [G,5], G)."""
        mo = check_model_of(model_of, n_env, self.n_models)
        key = mo.tobytes()
        hit = self._plans.get(key)
        if hit is None:
            cap = (n_env + 3) // 4 + self.n_models
            table = np.empty((cap, 5), dtype=np.int32)
            vp = ctypes.c_void_p
            g = self._L.pgp_gobi_plan_groups(n_env, mo.ctypes.data_as(vp), self.n_models, table.ctypes.data_as(vp), cap)
            if g < 0:
                raise RuntimeError(f"pgp_gobi_plan_groups: {g} {self._L.pgp_gobi_last_error().decode()}")
            if len(self._plans) >= 16:   # a fleet has a few assignments; do not grow without bound
                self._plans.clear()
            hit = self._plans[key] = (torch.as_tensor(table[:g].copy()).to(self.device), g)
        return hit

    def optimize(self, init, out=None, stream=None, max_iters=0, pre=None, model_of=None, groups=None):
        """init: [E,16,18] float32 (device tensor or host array).  max_iters /
        pre [E,16,16]: test hooks (step limit, pre-projection values).
        model_of: int [E], environment e's surrogate (None: all on model 0);
        its group table is planned once per content.  groups: a ready device
        table [G,5] int32 instead (see pgp_gobi_optimize_groups)."""
        x = torch.as_tensor(init, dtype=torch.float32).to(self.device).contiguous()
        if x.dim() != 3 or tuple(x.shape[1:]) != (H, H + 2):
            raise ValueError(f"init must be [E,{H},{H + 2}], got {tuple(x.shape)}")
        E = x.shape[0]
        if out is None:
            out = (torch.empty_like(x), torch.empty(E, dtype=torch.int32, device=self.device),
                   torch.empty(E, dtype=torch.float32, device=self.device))
        res, its, fit = out
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if model_of is not None and groups is not None:
            raise ValueError("model_of or groups, not both")
        if model_of is not None or groups is not None:
            if groups is None:
                groups, g = self.plan(model_of, E)
            else:
                if groups.dtype != torch.int32 or groups.dim() != 2 or groups.shape[1] != 5 or not groups.is_cuda:
                    raise ValueError("groups must be a device int32 tensor [G,5]")
                groups, g = groups.contiguous(), int(groups.shape[0])
            rc = self._L.pgp_gobi_optimize_groups(self._h, E, g, groups.data_ptr(), x.data_ptr(), res.data_ptr(),
                                                  its.data_ptr(), fit.data_ptr(), int(max_iters),
                                                  None if pre is None else pre.data_ptr(),
                                                  ctypes.c_void_p(st.cuda_stream))
            if rc != 0:
                raise RuntimeError(f"pgp_gobi_optimize_groups: {rc} {self._L.pgp_gobi_last_error().decode()}")
            return res, its, fit
        rc = self._L.pgp_gobi_optimize(self._h, E, x.data_ptr(), res.data_ptr(), its.data_ptr(), fit.data_ptr(),
                                       int(max_iters), None if pre is None else pre.data_ptr(),
                                       ctypes.c_void_p(st.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"pgp_gobi_optimize: {rc} {self._L.pgp_gobi_last_error().decode()}")
        return res, its, fit

    def optimize_so(self, init, out=None, stream=None, max_iters=0, signs=None, seeds=None, taps=None, model_of=None,
                    groups=None):
        """Batched so_opt() (scheduler/BaGTI/src/opt.py:35-51, Adahessian:
        scheduler/BaGTI/src/adahessian.py:49-168): optimize()'s shapes, result
        and model_of / groups.  Each step probes the Hessian with one +-1 per
        input entry; exactly one of
          signs: uint32 [E, steps, 9] (pack_signs; steps >= the step limit),
          seeds: integer [E] (a 64-bit device tensor is used where it is),
                 environment e's probes are so_signs(seeds[e:e+1], steps).
        max_iters / taps [E,3,16,18] (the last executed step's g, hv and
        pre-projection x): test hooks."""
        x = torch.as_tensor(init, dtype=torch.float32).to(self.device).contiguous()
        if x.dim() != 3 or tuple(x.shape[1:]) != (H, H + 2):
            raise ValueError(f"init must be [E,{H},{H + 2}], got {tuple(x.shape)}")
        E = x.shape[0]
        if (signs is None) == (seeds is None):
            raise ValueError("signs (explicit probes) or seeds (generated), not both")
        sign_steps = 0
        if signs is not None:
            if isinstance(signs, np.ndarray):
                signs = torch.as_tensor(signs.view(np.int32))
            signs = signs.to(self.device).contiguous()
            if signs.dim() != 3 or signs.shape[0] != E or signs.shape[2] != 9 or signs.element_size() != 4:
                raise ValueError(f"signs must be 32-bit words [{E}, steps, 9], got {tuple(signs.shape)}")
            sign_steps = int(signs.shape[1])
        else:
            if isinstance(seeds, torch.Tensor) and seeds.is_cuda:   # device-resident seeds: used where they are
                if seeds.dtype not in (torch.int64, torch.uint64) or tuple(seeds.shape) != (E,):
                    raise ValueError(f"seeds must be {E} 64-bit integers, got {seeds.dtype} {tuple(seeds.shape)}")
                seeds = seeds.to(self.device).contiguous()
            else:
                seeds = _seeds_u64(seeds)
                if seeds.shape != (E,):
                    raise ValueError(f"seeds must be {E} integers, got {seeds.shape[0]}")
                seeds = torch.as_tensor(seeds.view(np.int64)).to(self.device)
        if taps is not None and (taps.dtype != torch.float32 or tuple(taps.shape) != (E, 3, H, H + 2)
                                 or not taps.is_cuda or not taps.is_contiguous()):
            raise ValueError(f"taps must be a contiguous device float32 tensor [{E},3,{H},{H + 2}]")
        if out is None:
            out = (torch.empty_like(x), torch.empty(E, dtype=torch.int32, device=self.device),
                   torch.empty(E, dtype=torch.float32, device=self.device))
        res, its, fit = out
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if model_of is not None and groups is not None:
            raise ValueError("model_of or groups, not both")
        tail = (int(max_iters), None if signs is None else signs.data_ptr(), sign_steps,
                None if seeds is None else seeds.data_ptr(), None if taps is None else taps.data_ptr(),
                ctypes.c_void_p(st.cuda_stream))
        if model_of is not None or groups is not None:
            if groups is None:
                groups, g = self.plan(model_of, E)
            else:
                if groups.dtype != torch.int32 or groups.dim() != 2 or groups.shape[1] != 5 or not groups.is_cuda:
                    raise ValueError("groups must be a device int32 tensor [G,5]")
                groups, g = groups.contiguous(), int(groups.shape[0])
            rc = self._L.pgp_gobi_so_optimize_groups(self._h, E, g, groups.data_ptr(), x.data_ptr(), res.data_ptr(),
                                                     its.data_ptr(), fit.data_ptr(), *tail)
            what = "pgp_gobi_so_optimize_groups"
        else:
            rc = self._L.pgp_gobi_so_optimize(self._h, E, x.data_ptr(), res.data_ptr(), its.data_ptr(),
                                              fit.data_ptr(), *tail)
            what = "pgp_gobi_so_optimize"
        if rc != 0:
            raise RuntimeError(f"{what}: {rc} {self._L.pgp_gobi_last_error().decode()}")
        return res, its, fit

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.pgp_gobi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scheduler:
    """The scheduler plugin interface COSCO drives (scheduler/Scheduler.py:9-38):
    main.py:154-155 calls ``selection()``, ``placement(ids)`` and
    ``filter_placement(decision)``; Simulator.py:118, 173-174 call
    ``getMigrationFromHost`` / ``getMigrationToHost``.  Only these plugin methods
    are restated; the base class's host-selection heuristics (LR / MAD / IQR
    ..., :40-185) belong to the other schedulers, which are out of scope."""

    def __init__(self):
        self.env = None

    def setEnvironment(self, env):
        self.env = env

    def selection(self):
        return None

    def placement(self, containerlist):
        return None

    def filter_placement(self, decision):
        """Scheduler.py:20-25: drop decisions that keep a container in place."""
        return [(cid, hid) for cid, hid in decision if self.env.getContainerByID(cid).getHostID() != hid]

    def getMigrationFromHost(self, hostID, decision):
        """Scheduler.py:27-32."""
        return [cid for cid, _ in decision if self.env.getContainerByID(cid).getHostID() == hostID]

    def getMigrationToHost(self, hostID, decision):
        """Scheduler.py:34-38."""
        return [cid for cid, hid in decision if hid == hostID]


class GOBIScheduler(Scheduler):
    """The placement step of scheduler/GOBI.py:19-48 on the COSCO env interface
    (hostlist[i].getCPU(), containerlist[c].getApparentIPS() / getHostID() / id),
    a drop-in for the scheduler main.py builds (``GOBIScheduler('energy_latency_16')``)."""

    def __init__(self, data_type="energy_latency_16", device="cuda", weights=None, max_ips=None):
        """weights / max_ips: a surrogate trained on the environment's own
        traces (gobitrain.GOBITrainer.weights_numpy() and the max_ips of
        gobitrain.load_energy_latency_data); both or neither.  None: the
        packaged copy of the reference's checkpoint."""
        super().__init__()
        if data_type != "energy_latency_16":
            raise ValueError("only the energy_latency_16 surrogate ships with the reference")
        if (weights is None) != (max_ips is None):
            raise ValueError("a trained surrogate comes with its dataset's max_ips: pass weights and max_ips together")
        self.opt = GOBIOptimizer(weights=weights, device=device)
        self.max_container_ips = self.opt.max_ips if max_ips is None else float(max_ips)
        self.data_type = data_type
        self.hosts = H
        self.result_cache = None

    def selection(self):
        """GOBI.py:44-45: GOBI re-places every container, it selects none."""
        return []

    def init_matrix(self, rng=np.random):
        """GOBI.py:20-32: [host cpu / 100, container ips / max, one-hot host];
        an unplaced container gets a random host, as the reference draws it."""
        cpu = np.array([[h.getCPU() / 100 for h in self.env.hostlist]]).T
        cpuc = np.array([[(c.getApparentIPS() / self.max_container_ips if c else 0) for c in self.env.containerlist]]).T
        alloc, prev = [], {}
        for c in self.env.containerlist:
            one = [0] * len(self.env.hostlist)
            if c:
                prev[c.id] = c.getHostID()
            if c and c.getHostID() != -1:
                one[c.getHostID()] = 1
            else:
                one[rng.randint(0, len(self.env.hostlist))] = 1
            alloc.append(one)
        return np.concatenate((cpu, cpuc, np.array(alloc)), axis=1), prev

    def _optimize(self, init):
        return self.opt.optimize(init)

    def run_GOBI(self):
        init, prev = self.init_matrix()
        res, _, _ = self._optimize(init[None])
        result = res[0].cpu().numpy()
        self.result_cache = result[:, -self.hosts:]
        decision = []
        for cid in prev:  # GOBI.py:37-41
            one_hot = result[cid, -self.hosts:].tolist()
            new_host = one_hot.index(max(one_hot))
            if prev[cid] != new_host:
                decision.append((cid, new_host))
        return decision

    def placement(self, containerIDs):
        return self.run_GOBI()


class SOGOBIScheduler(GOBIScheduler):
    """scheduler/SOGOBI.py:8-48: GOBIScheduler with the second-order optimiser
    (run_SOGOBI's so_opt, SOGOBI.py:34).  run_GOBI, result_cache and the
    decision list are GOBIScheduler's.  The reference draws its Hutchinson
    probes from torch's global generator; here call n (from 0) of a scheduler
    built with ``seed`` draws them from the per-call seed ``call_seed(n)``, so
    a run is reproducible and two schedulers with different seeds are
    independent."""

    def __init__(self, data_type="energy_latency_16", device="cuda", weights=None, max_ips=None, seed=0):
        super().__init__(data_type, device=device, weights=weights, max_ips=max_ips)
        self.seed = int(seed)
        self.calls = 0

    def call_seed(self, n):
        """The 64-bit probe seed of call n: the scheduler's seed in the high word, the call in the low."""
        return ((self.seed & 0xFFFFFFFF) << 32) | (int(n) & 0xFFFFFFFF)

    def _optimize(self, init):
        seeds = np.array([self.call_seed(self.calls)], dtype=np.uint64)
        self.calls += 1
        return self.opt.optimize_so(init, seeds=seeds)

    run_SOGOBI = GOBIScheduler.run_GOBI
