"""The AdamW kernels alone (csrc/pgp_train.hip: ``adamw_kernel``,
``adamw_cells_kernel``, and ``adamw_update`` of pgp_train.hpp they share with
every fused step) on prescribed gradients, through the C-ABI entries
pgp_adamw_d, pgp_adamw_table_d and pgp_adamw_table_many_d (the betas as doubles:
the entries the package calls), against the fp64 replay and the rounding bound
of tests/adamw_replay.py.  The float-beta entries of the same names without the
suffix are held, bit for bit, to their definition: the _d entry at the betas
rounded to fp32.

Every buffer holds 40,000 floats.  The tensors lie in its first quarter (the
"chunks" table's named lengths add up to 9,947 elements), so three quarters of
each buffer are sentinels that must keep their bits.

The fused steps that carry the same update are replayed from the ``G`` they
leave behind in tests/test_gpu_adamw_fused.py (``pgp_online_step`` among them:
test_gpu_c3step.py::test_native_step_equals_python_composition pins it bitwise
to the Python composition of these entries, and one small replay covers the
update fused into its GAN kernels).  Out of scope of both: GOBI's coupled-L2
Adam, which exposes no ``G`` (tests/test_gpu_gobitrain.py::test_gradient_alone)."""
import numpy as np
import pytest
import torch

from preganplus_amd import _native
from preganplus_amd import train as TR
from tests import adamw_replay as AR

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FC0DEAD], dtype=np.uint32).view(np.float32)[0]      # a NaN no update leaves in place by luck
# at kAdamChunk = 1024 and at the 256-thread block; a zero-length tensor in the middle
LENGTHS = (1, 255, 256, 257, 1023, 0, 1024, 1025, 2049, 4097)
MAX_TENSORS = 48
BUFFER = 40_000


def layout(lengths, gap0=5):
    """Tensors back to back with gaps of 5, 6, 7, ... floats in front of each (odd offsets): [(offset, n)], extent."""
    out, off = [], 0
    for i, n in enumerate(lengths):
        off += gap0 + i % 4
        out.append((off, n))
        off += n
    return out, off + gap0


TABLES = {
    "chunks": (LENGTHS, None),                                              # every tensor active
    "many_small": (tuple(1 + i % 3 for i in range(MAX_TENSORS)), None),     # kMaxTensors tensors of 1-3 elements
    "alternate": (LENGTHS, tuple(i % 2 for i in range(len(LENGTHS)))),      # inactive, active, inactive, ...
}


def make(table, step, seed, hyper="project"):
    """Host arrays of one case: P / m / v / G with sentinels in every gap, the
    tensor list [(offset, n, active, step)]."""
    lengths, act = TABLES[table]
    lay, extent = layout(lengths)
    assert extent <= BUFFER
    extent = BUFFER
    P, m, v, G = AR.synthetic(extent, seed, fresh=step == 1)
    gap = np.ones(extent, dtype=bool)
    for off, n in lay:
        gap[off:off + n] = False
    for a in (P, m, v, G):
        a[gap] = SENTINEL
    tensors = [(off, n, 1 if act is None else act[i], step) for i, (off, n) in enumerate(lay)]
    return {"P": P, "m": m, "v": v, "G": G}, tensors


def up(host):
    return {k: torch.from_numpy(a.copy()).cuda() for k, a in host.items()}


def down(dev):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in dev.items()}


def rows(tensors, hy):
    """The device table rows (active, step_size, bc2_sqrt) of a tensor list, as Trainer.adam_schedule_np writes them."""
    return np.array([[float(a), hy["lr"] / (1 - hy["b1"] ** max(s, 1)), np.sqrt(1 - hy["b2"] ** max(s, 1))]
                     for _, _, a, s in tensors], dtype=np.float32)


def hyper_args(hy):
    return hy["lr"], hy["wd"], hy["b1"], hy["b2"], hy["eps"]


def run_entry(entry, dev, tensors, hy, float_betas=False, rows_hy=None):
    """entry: "pgp_adamw" (host scalars) or "pgp_adamw_table" (device rows), through the _d form, or with
    ``float_betas`` through the float-beta form; rows_hy: the hyper-parameters the per-step scalars come from
    (default hy)."""
    L = _native.lib()
    sfx = "" if float_betas else "_d"
    p = lambda k: dev[k].data_ptr()
    T = len(tensors)
    tab = rows(tensors, rows_hy or hy)
    if entry == "pgp_adamw":             # host scalars
        desc = (TR._AdamTensor * T)(*[TR._AdamTensor(o, n, a, float(tab[i, 1]), float(tab[i, 2]))
                                      for i, (o, n, a, _) in enumerate(tensors)])
        _native.check(getattr(L, entry + sfx)(p("P"), p("G"), p("m"), p("v"), *hyper_args(hy), desc, T, None), entry)
    else:                                # device rows; the descriptor's own fields must not matter
        desc = (TR._AdamTensor * T)(*[TR._AdamTensor(o, n, 1, 7.0, 0.5) for o, n, _, _ in tensors])
        sched = torch.from_numpy(tab).cuda()
        _native.check(getattr(L, entry + sfx)(p("P"), p("G"), p("m"), p("v"), *hyper_args(hy), desc, T,
                                              sched.data_ptr(), None), entry)
    torch.cuda.synchronize()


def record(key, worst):
    print(f"AdamW {key}: worst error/tolerance P {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


@pytest.mark.parametrize("step", AR.STEPS)
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("entry", ["pgp_adamw", "pgp_adamw_table"])
def test_update_inside_bounds(entry, table, step):
    hyper = "decay" if step == 10 else "project"
    hy = AR.HYPERS[hyper]
    host, tensors = make(table, step, seed=100 * step + len(table))
    if table == "alternate":
        assert {a for _, _, a, _ in tensors} == {0, 1}
    dev = up(host)
    run_entry(entry, dev, tensors, hy)
    record(f"{entry} {table} step {step}", AR.assert_step(f"{entry} {table} step {step}", host, down(dev), tensors, **hy))


@pytest.mark.parametrize("entry", ["pgp_adamw", "pgp_adamw_table"])
def test_chained_steps_do_not_drift(entry):
    """20 steps from zero moments, a new prescribed gradient each, every step
    checked from the kernel's own state before it."""
    hy = AR.HYPERS["project"]
    host, tensors = make("chunks", 1, seed=7)
    dev = up(host)
    act = AR.active_mask(host["G"].size, tensors)
    worst = np.zeros(3)
    for step in range(1, 21):
        before = down(dev)
        G = AR.synthetic(before["G"].size, 300 + step, fresh=True)[3]
        before["G"] = np.where(act, G, before["G"])
        dev["G"].copy_(torch.from_numpy(before["G"]))
        ts = [(o, n, a, step) for o, n, a, _ in tensors]
        run_entry(entry, dev, ts, hy)
        worst = np.maximum(worst, AR.assert_step(f"{entry} chained step {step}", before, down(dev), ts, **hy))
    record(f"{entry} 20 chained steps", worst)


def test_zero_length_tensor_is_accepted():
    """n = 0 in the middle of a table owns no block of the flat grid (LENGTHS has one, so every "chunks" case
    above runs through it); alone it launches nothing and returns PGP_OK."""
    assert 0 in LENGTHS[1:-1]
    host, _ = make("chunks", 2, seed=3)
    dev = up(host)
    tensors = [(17, 0, 1, 2)]
    run_entry("pgp_adamw", dev, tensors, AR.HYPERS["project"])
    run_entry("pgp_adamw_table", dev, tensors, AR.HYPERS["project"])
    after = down(dev)
    for k in host:
        assert np.array_equal(AR.bits(after[k]), AR.bits(host[k])), k


def test_table_many_cells():
    """pgp_adamw_table_many: 3 cells, cell 1 inactive (its rows say active: the cell flag rules), a slot stride
    larger than the tensors' extent, a table stride larger than the table, each cell at its own step count, and
    one table row of an active cell with active = 0."""
    L = _native.lib()
    hy = AR.HYPERS["project"]
    cell_steps = (2, 7, 10000)
    lengths, _ = TABLES["chunks"]
    lay, _ = layout(lengths)
    extent = BUFFER
    slot_len = extent + 333
    T = len(lay)
    tab_stride = 3 * T + 5
    hosts, tens = [], []
    tab = np.full((3, tab_stride), SENTINEL, dtype=np.float32)
    for c, step in enumerate(cell_steps):
        h, ts = make("chunks", step, seed=40 + c)
        if c == 2:
            ts[3] = ts[3][:2] + (0,) + ts[3][3:]              # a row with active = 0 in an active cell
        hosts.append({k: np.concatenate([a, np.full(slot_len - extent, SENTINEL, dtype=np.float32)])
                      for k, a in h.items()})
        tab[c, :3 * T] = rows(ts, hy).reshape(-1)
        tens.append(ts)
    host = {k: np.concatenate([h[k] for h in hosts]) for k in "PmvG"}
    dev = up(host)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    sched = torch.from_numpy(tab).cuda()
    desc = (TR._AdamTensor * T)(*[TR._AdamTensor(o, n, 1, 7.0, 0.5) for o, n in lay])
    p = lambda k: dev[k].data_ptr()
    _native.check(L.pgp_adamw_table_many_d(3, slot_len, active.data_ptr(), p("P"), p("G"), p("m"), p("v"),
                                         *hyper_args(hy), desc, T, sched.data_ptr(), tab_stride, None),
                  "pgp_adamw_table_many")
    after = down(dev)
    assert np.array_equal(AR.bits(sched.cpu().numpy()), AR.bits(tab))
    flat = [(c * slot_len + o, n, a if c != 1 else 0, s) for c, ts in enumerate(tens) for o, n, a, s in ts]
    record("pgp_adamw_table_many", AR.assert_step("pgp_adamw_table_many", host, after, flat, **hy))
    # every cell flag NULL: all three cells step
    dev = up(host)
    _native.check(L.pgp_adamw_table_many_d(3, slot_len, None, p("P"), p("G"), p("m"), p("v"), *hyper_args(hy), desc, T,
                                         sched.data_ptr(), tab_stride, None), "pgp_adamw_table_many")
    flat = [(c * slot_len + o, n, a, s) for c, ts in enumerate(tens) for o, n, a, s in ts]
    record("pgp_adamw_table_many (no cell flags)",
           AR.assert_step("pgp_adamw_table_many, active NULL", host, down(dev), flat, **hy))
    # a tensor that leaves the slot is refused before anything runs
    bad = (TR._AdamTensor * 1)(TR._AdamTensor(slot_len - 1, 2, 1, 0.0, 0.0))
    dev = up(host)
    rc = L.pgp_adamw_table_many_d(3, slot_len, None, p("P"), p("G"), p("m"), p("v"), *hyper_args(hy), bad, 1,
                                sched.data_ptr(), tab_stride, None)
    assert _native._ERRS.get(rc) == "PGP_ERR_ARG"
    after = down(dev)
    for k in host:
        assert np.array_equal(AR.bits(after[k]), AR.bits(host[k])), k


def test_three_entries_agree_across_the_block_edge():
    """pgp_adamw_d, pgp_adamw_table_d and pgp_adamw_table_many_d leave identical bits on one tensor list whose
    lengths straddle the 1024-element block (1, 1023, 1025, 2048: the smallest at which a wrong block -> tensor
    lookup or a wrong slot offset shows), one step; the fleet entry with a second, inactive cell that keeps its
    bits.  The step itself is held to the replay's bound."""
    L = _native.lib()
    hy = AR.HYPERS["project"]
    lay, slot_len = layout((1, 1023, 1025, 2048))
    tensors = [(o, n, 1, 3) for o, n in lay]
    T = len(tensors)
    cells = []
    for seed in (61, 62):
        h = dict(zip("PmvG", AR.synthetic(slot_len, seed, fresh=False)))
        gap = ~AR.active_mask(slot_len, tensors)
        for a in h.values():
            a[gap] = SENTINEL
        cells.append(h)
    out = {}
    for entry in ("pgp_adamw", "pgp_adamw_table"):
        dev = up(cells[0])
        run_entry(entry, dev, tensors, hy)
        out[entry] = down(dev)
    record("block edge", AR.assert_step("pgp_adamw, block edge", cells[0], out["pgp_adamw"], tensors, **hy))
    host = {k: np.concatenate([c[k] for c in cells]) for k in "PmvG"}
    dev = up(host)
    active = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    sched = torch.from_numpy(np.stack([rows(tensors, hy)] * 2)).cuda()     # cell 1's rows say active: its flag rules
    desc = (TR._AdamTensor * T)(*[TR._AdamTensor(o, n, 1, 7.0, 0.5) for o, n in lay])
    _native.check(L.pgp_adamw_table_many_d(2, slot_len, active.data_ptr(), *(dev[k].data_ptr() for k in "PGmv"),
                                           *hyper_args(hy), desc, T, sched.data_ptr(), 3 * T, None),
                  "pgp_adamw_table_many")
    many = down(dev)
    for k in "PmvG":
        assert np.array_equal(AR.bits(out["pgp_adamw_table"][k]), AR.bits(out["pgp_adamw"][k])), k
        assert np.array_equal(AR.bits(many[k][:slot_len]), AR.bits(out["pgp_adamw"][k])), k
        assert np.array_equal(AR.bits(many[k][slot_len:]), AR.bits(cells[1][k])), k


@pytest.mark.parametrize("entry", ["pgp_adamw", "pgp_adamw_table", "pgp_adamw_table_many"])
def test_float_beta_entries_are_the_double_entries_at_rounded_betas(entry):
    """The entries that take the betas as floats stay as first exported: each is its _d form at
    (double)(float)beta, bit for bit in all four buffers, and so NOT torch's moment weights (1 - 0.999f is
    1.29e-5 from 1 - 0.999: outside the replay's bound, which is why the package calls the _d forms)."""
    L = _native.lib()
    hy = AR.HYPERS["project"]
    rounded = dict(hy, b1=float(np.float32(hy["b1"])), b2=float(np.float32(hy["b2"])))
    host, tensors = make("chunks", 10, seed=11)
    out = []
    for h, as_float in ((hy, True), (rounded, False)):    # the per-step scalars from the exact betas in both
        dev = up(host)
        if entry == "pgp_adamw_table_many":
            T = len(tensors)
            desc = (TR._AdamTensor * T)(*[TR._AdamTensor(o, n, 1, 0.0, 0.0) for o, n, _, _ in tensors])
            sched = torch.from_numpy(rows(tensors, hy)).cuda()
            f = L.pgp_adamw_table_many if as_float else L.pgp_adamw_table_many_d
            _native.check(f(1, BUFFER, None, *(dev[k].data_ptr() for k in "PGmv"), *hyper_args(h), desc, T,
                            sched.data_ptr(), 3 * T, None), entry)
        else:
            run_entry(entry, dev, tensors, h, float_betas=as_float, rows_hy=hy)
        out.append(down(dev))
    for k in "PGmv":
        assert np.array_equal(AR.bits(out[0][k]), AR.bits(out[1][k])), k
    assert not np.array_equal(AR.bits(out[0]["P"]), AR.bits(host["P"]))
    # and the float form is outside the bound torch's weights define
    r = AR.ratios([out[0][k] for k in "Pmv"], host["P"], host["m"], host["v"], host["G"], tensors, **hy)
    assert max(x.max() for x in r) > 1
