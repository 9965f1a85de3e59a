"""Host side of data-parallel training: the loader's global-batch sharding (``shard_mode="batch"``, csbsr_amd/data/resident.py), do_train /
validate / save_checkpoint / resume over two gloo ranks (csbsr_amd/trainer.py) and the argument checks of csbsr_amd.parallel.agree.

The trainer runs over a stub with the model's surface, in fp64, whose per-sample losses are a function of the sample (and of two weights
that SGD moves): sample values, learning rate and loss weight are dyadic, so every batch mean is exact in fp32 as well as in fp64 and the
one-process run over global batches of 2 b is a reference to the last bit, not to a rounding.  The device fingerprint has no host fallback;
the two ranks run the numpy restatement (tests/fingerprint_cases.py) in its place, so the MIN / MAX comparison and everything after it is
the shipped code."""
import datetime
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fingerprint_cases as FC
import resident_cases as RC

SIZES13 = [(40, 52), (31, 45), (24, 32), (50, 33), (37, 64), (33, 33), (48, 29), (26, 26), (64, 40), (29, 51), (36, 36), (45, 27), (30, 60)]
RESIZED = {"scale": (0.3, 1.0), "ratio": (0.75, 1.25)}


def _dataset(sizes):
    from csbsr_amd.data import resident as R
    images, masks = RC.random_pairs(np.random.default_rng(0), sizes)
    return R, R.ResidentDataset(images, masks, device="cpu")


def _same(a, b):
    return a[0].dtype == b[0].dtype and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _state_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


# ----------------------------------------------------------------------------------------------------------------- 1. the loader
@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized_crop"])
@pytest.mark.parametrize("world", [2, 3])
def test_batch_mode_ranks_concatenate_to_the_single_loader(world, resized):
    R, ds = _dataset(SIZES13)
    b = 2
    G = world * b
    kw = dict(seed=17, drop_last=True, vflip_p=0.3, resized_crop=RESIZED if resized else None)
    n = 3 * (13 // G)                                            # three epochs of whole global batches
    single = R.DeviceTrainLoader(ds, 16, 4, batch_size=G, num_iterations=n, **kw)
    ranks = [R.DeviceTrainLoader(ds, 16, 4, batch_size=b, num_iterations=n, shard=(r, world), shard_mode="batch", **kw) for r in range(world)]
    assert all(len(ld) == n == len(single) for ld in ranks)
    its = [ld.iter_decisions() for ld in ranks]
    steps = 0
    for sel, params in single.iter_decisions():
        got = [next(it) for it in its]
        assert all(g[0].shape == (b, 7 if resized else 5) and g[1].shape == (b, 3) for g in got)
        assert _same((torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), (sel, params))
        states = [ld.state_dict() for ld in ranks]
        for st in states[1:]:
            _state_equal(states[0], st)
        assert states[0]["global_batch"] == G and states[0]["produced"] == single.produced == ranks[-1].produced
        assert torch.equal(states[0]["generator"], single.state_dict()["generator"])          # the generator advanced as the single loader's
        steps += 1
    assert steps == n and all(next(it, "end") == "end" for it in its)
    assert sorted(set(torch.cat([s[:, 0] for s, _ in single.iter_decisions()]).tolist())) == list(range(13))      # (over the WHOLE dataset)


def test_batch_mode_state_continues_on_another_world_size():
    R, ds = _dataset(SIZES13)
    mk = lambda b, shard, seed=5: R.DeviceTrainLoader(ds, 16, 4, batch_size=b, num_iterations=9, seed=seed, drop_last=True, shard=shard,
                                                      shard_mode="batch")
    whole = list(R.DeviceTrainLoader(ds, 16, 4, batch_size=4, num_iterations=9, seed=5, drop_last=True).iter_decisions())
    two = [mk(2, (r, 2)) for r in range(2)]
    its = [ld.iter_decisions() for ld in two]
    for _ in range(4):                                           # past the first epoch boundary (three global batches of 13 images)
        for it in its:
            next(it)
    state = two[1].state_dict()
    four = [mk(1, (r, 4), seed=999) for r in range(4)]
    for ld in four:
        ld.load_state_dict(state)
    tails = [list(ld.iter_decisions()) for ld in four]
    assert all(len(t) == 5 for t in tails) and all(ld.produced == 9 for ld in four)
    for step in range(5):
        assert _same((torch.cat([t[step][0] for t in tails]), torch.cat([t[step][1] for t in tails])), whole[4 + step])
    # another global batch, or a state of the other mode, is refused
    with pytest.raises(ValueError):
        mk(2, (0, 4)).load_state_dict(state)
    with pytest.raises(ValueError):
        mk(1, (0, 2)).load_state_dict(state)
    sample = R.DeviceTrainLoader(ds, 16, 4, batch_size=4, num_iterations=9, seed=5, drop_last=True)
    with pytest.raises(ValueError):
        mk(4, (0, 1)).load_state_dict(sample.state_dict())
    with pytest.raises(ValueError):
        sample.load_state_dict(state)
    assert "global_batch" not in sample.state_dict()


def test_batch_mode_needs_equal_shards_when_shuffling():
    R, ds = _dataset(SIZES13)
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=1, shard=(0, 2), shard_mode="batch")                   # shuffle=True, drop_last=False
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=1, num_iterations=8, shard=(1, 2), shard_mode="batch")
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=1, shard=(0, 2), shard_mode="rows")
    R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=1, shard=(0, 1), shard_mode="batch")                       # one rank: nothing to keep equal
    R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=1, shard=(0, 2), shard_mode="batch", drop_last=True)
    R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=1, shard=(0, 2), shard_mode="batch", shuffle=False)


def test_batch_mode_sequential_pass_splits_the_short_batch_contiguously():
    R, ds = _dataset(SIZES13[:5])
    view = ds.subset([4, 0, 3, 1, 2])
    single = list(R.DeviceTrainLoader(view, 16, 4, batch_size=4, seed=3, shuffle=False).iter_decisions())
    ranks = [R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=3, shuffle=False, shard=(r, 2), shard_mode="batch") for r in range(2)]
    got = [list(ld.iter_decisions()) for ld in ranks]
    assert [len(ld) for ld in ranks] == [2, 2] and [len(g) for g in got] == [2, 2]
    assert [None if g is None else g[0].shape[0] for g in got[0]] == [2, 1]
    assert [None if g is None else g[0].shape[0] for g in got[1]] == [2, None]
    assert got[0][0][0][:, 0].tolist() == [4, 0] and got[1][0][0][:, 0].tolist() == [3, 1] and got[0][1][0][:, 0].tolist() == [2]
    assert _same((torch.cat([got[0][0][0], got[1][0][0]]), torch.cat([got[0][0][1], got[1][0][1]])), single[0])
    assert _same(got[0][1], single[1])
    _state_equal(ranks[0].state_dict(), ranks[1].state_dict())
    assert [ld.produced for ld in ranks] == [2, 2]


# recorded from the loader before shard_mode existed: seven images, shard (1, 2), b = 2, seed 11, four batches (epochs of 2 + 1 samples)
_PIN_SEL = [[[1, 14, 20, 0, 0], [5, 2, 3, 1, 0]], [[3, 25, 8, 1, 1]], [[3, 19, 9, 0, 0], [5, 9, 14, 1, 0]], [[1, 15, 11, 1, 0]]]
_PIN_BLUR = [["0x1.a0715a0000000p+1", "0x1.8dd7200000000p+1", "0x1.5e36040000000p+1", "0x1.794b400000000p+1", "0x1.b0710a0000000p+1",
              "0x1.d4175c0000000p+0"], ["0x1.205f7c0000000p+0", "0x1.7c2cf40000000p+0", "0x1.63c6540000000p+1"],
             ["0x1.8e22e80000000p+0", "0x1.04958e0000000p+1", "0x1.0f834a0000000p+1", "0x1.28cb600000000p+0", "0x1.1a02540000000p+1",
              "0x1.4d00260000000p+1"], ["0x1.6820160000000p+1", "0x1.c24cc80000000p+0", "0x1.0354240000000p+1"]]
_PIN_WINDOWS = [[[1, 4, 18, 0, 0, 26, 22], [5, 1, 0, 1, 1, 31, 33]], [[3, 3, 4, 0, 0, 36, 28]], [[3, 18, 0, 0, 1, 31, 26], [1, 0, 0, 0, 0, 31, 29]],
                [[5, 0, 0, 1, 0, 30, 30]]]


def test_sample_mode_is_the_default_and_its_sequence_is_unchanged():
    R, ds = _dataset(SIZES13[:7])
    for kw in ({}, {"shard_mode": "sample"}):
        ld = R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=11, num_iterations=4, shard=(1, 2), vflip_p=0.3, **kw)
        out = list(ld.iter_decisions())
        assert [s.tolist() for s, _ in out] == _PIN_SEL and all(s.dtype == torch.int32 for s, _ in out)
        assert [[float(v).hex() for v in p.reshape(-1)] for _, p in out] == _PIN_BLUR
        assert sorted(ld.state_dict()) == ["cursor", "generator", "perm", "produced", "samples"] and ld.state_dict()["samples"] == 3
        assert len(ld) == 4 and ld.shard_mode == "sample"
    ld = R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=11, num_iterations=4, shard=(1, 2), vflip_p=0.3, resized_crop=RESIZED)
    assert [s.tolist() for s, _ in ld.iter_decisions()] == _PIN_WINDOWS


# ----------------------------------------------------------------------------------------------------------------- 2. agree: arguments
def test_fingerprint_refuses_what_the_kernel_cannot_read():
    from csbsr_amd import _lib as L
    from csbsr_amd.parallel import agree
    with pytest.raises(ValueError):
        agree.fingerprint([torch.zeros(4, 6)[:, ::2]])                             # not contiguous
    with pytest.raises(ValueError):
        agree.fingerprint([torch.zeros(3, dtype=torch.uint8)])                     # 3 bytes: not a whole number of words
    with pytest.raises(ValueError):
        agree.fingerprint([torch.zeros(5, dtype=torch.float16)])                   # 10 bytes
    with pytest.raises(ValueError):
        agree.fingerprint([])
    with pytest.raises(ValueError):
        agree.fingerprint([np.zeros(4, np.float32)])
    with pytest.raises(L.CsbsrHipError):
        agree.fingerprint([torch.zeros(8)])                                        # a host tensor: no fallback
    with pytest.raises(L.CsbsrHipError):
        agree.replicas_agree({"w": torch.zeros(8)})
    with pytest.raises(L.CsbsrHipError):
        agree.assert_replicas_agree([("w", torch.zeros(2, dtype=torch.int64))])
    assert agree.replicas_agree({}) == []
    assert issubclass(agree.ReplicaMismatch, RuntimeError)


# ----------------------------------------------------------------------------------------------------------------- 3. the trainer, two ranks
B_RANK, WORLD, IT0 = 2, 2, 8          # iterations 9 .. 12: windows close at 10 and 12, validation runs at 12


class _Alpha:
    def __init__(self):
        self.alpha, self.iter, self.fix_alpha = 1.0, 0, False

    def update_alpha(self):
        self.alpha -= 0.01


class _Stub(torch.nn.Module):
    """do_train's and validate's view of the model, in fp64: per-sample losses  s_i + w_0 t_i  and  r_i + w_1 q_i  of dyadic sample values"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.5, -0.25], dtype=torch.float64))
        self.register_buffer("steps_seen", torch.zeros(1, dtype=torch.int64))
        self.ss_loss_fn = _Alpha()
        self.iter_cnt, self.last_step_overflowed, self.reducer = True, False, None

    def forward(self, iter, x, sr_targets=None, segment_targets=None, kernel_targets=None, segment_sdf=None):
        if self.training:
            self.steps_seen += 1
        seg_loss = x.mean((1, 2, 3)) + self.w[0] * sr_targets.mean((1, 2, 3))
        sr_loss = kernel_targets.mean((1, 2, 3)) + self.w[1] * x.mean((1, 2, 3))
        return seg_loss, sr_loss, segment_targets * 0 + x.mean((1, 2, 3)).reshape(-1, 1, 1, 1), sr_targets * 0.5, kernel_targets * 0.75


class _SGD(torch.optim.SGD):
    """plain SGD; data-parallel, the gradients go through the reducer do_train attached to the model first (the real model's backward does
    that itself)"""

    def __init__(self, model, lr):
        super().__init__(model.parameters(), lr=lr)
        self.model = model

    def step(self, *a, **kw):
        red = self.model.reducer
        if red is not None:
            red.launch([p.grad for p in self.model.parameters()])
            red.finish()
        return super().step(*a, **kw)


class _HostBatches:
    """a DeviceTrainLoader's decisions turned into host batches that are a function of the selected rows alone (the device turns them into
    pixels): the trainer sees the loader's length, count, state and None items"""

    def __init__(self, loader):
        self.loader, self.gen, self.shard_mode = loader, loader.gen, loader.shard_mode

    def __len__(self):
        return len(self.loader)

    @property
    def produced(self):
        return self.loader.produced

    def state_dict(self):
        return self.loader.state_dict()

    def load_state_dict(self, state):
        self.loader.load_state_dict(state)

    @staticmethod
    def _make(sel, params):
        s = sel.to(torch.float64)
        plane = lambda v, c, n: (v % 64 / 64).reshape(-1, 1, 1, 1) * torch.ones(1, c, n, n, dtype=torch.float64)
        return (plane(s[:, 0] * 37 + s[:, 1] * 5 + s[:, 2], 3, 2), plane(s[:, 0] * 11 + s[:, 2] * 3 + s[:, 3], 3, 4),
                (plane(s[:, 1] * 7 + s[:, 0], 1, 4) > 0.5).double(), plane(s[:, 2] * 13 + s[:, 4] + s[:, 0], 1, 3))

    def __iter__(self):
        for item in self.loader.iter_decisions():
            yield None if item is None else self._make(*item)


def _cfg():
    from csbsr_amd.config import cfg
    c = cfg.clone()
    c.SOLVER.SR_PRETRAIN_ITER, c.SOLVER.TASK_LOSS_WEIGHT, c.SOLVER.LR = [0, 0], 0.5, 0.25
    return c


def _loaders(rank, world, b, n, seed=21, mode="batch"):
    R, ds = _dataset(SIZES13)
    train = R.DeviceTrainLoader(ds, 16, 4, batch_size=b, num_iterations=n, seed=seed, drop_last=True, shard=(rank, world), shard_mode=mode)
    _, ev = _dataset(SIZES13[:5])
    evl = R.DeviceTrainLoader(ev, 16, 4, batch_size=b, seed=4, shuffle=False, shard=(rank, world), shard_mode=mode)
    return _HostBatches(train), _HostBatches(evl)


def _host_metrics():
    from csbsr_amd.utils import estimate_metrics as EM
    EM.psnr_ssim = lambda a, b: (10 * torch.log10(1 / (((a - b) ** 2).mean((1, 2, 3)) + 1e-3)), (a * b).mean((1, 2, 3)))
    EM.iou_sweep = lambda p, m, thresholds, smooth=1e-5: ((((p > 0.5) & (m > 0.5)).sum((1, 2, 3)) + smooth)
                                                          / (((p > 0.5) | (m > 0.5)).sum((1, 2, 3)) + smooth)).reshape(-1, 1)


def _train(T, cfg, model, loaders, resume_iter, out_dir=None, opt=None, **kw):
    opt = _SGD(model, cfg.SOLVER.LR) if opt is None else opt
    logs, seen = [], []
    T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt, resume_iter), loaders[0], loaders[1], resume_iter=resume_iter, log_step=2,
               eval_step=4, output_dir=out_dir, log=logs.append, hooks={"after_step": lambda it, m, rec: seen.append(rec)}, **kw)
    strip = lambda r: None if r is None else {k: v for k, v in r.items() if k not in ("cost_s", "eta")}
    return [strip(r) for r in logs], [strip(r) for r in seen]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from csbsr_amd import trainer as T
    from csbsr_amd.parallel import agree
    from csbsr_amd.parallel.reducer import GradBucketReducer
    agree.fingerprint = lambda tensors: torch.from_numpy(FC.fingerprint_numpy([t.detach().numpy() for t in tensors]))
    _host_metrics()
    saves = []
    real_save = torch.save
    # files only: gather_object pickles through torch.save into a BytesIO
    torch.save = lambda obj, f, *a, **kw: (saves.append(str(f)) if isinstance(f, (str, os.PathLike)) else None, real_save(obj, f, *a, **kw))[1]
    cfg = _cfg()
    res = {}
    # (a) four iterations in one go; the replicas start from DIFFERENT weights and rank 0's win
    torch.manual_seed(100 + rank)
    full = _Stub()
    with torch.no_grad():
        full.w += rank
    res["full_logs"], res["full_seen"] = _train(T, cfg, full, _loaders(rank, world, B_RANK, 4), IT0, os.path.join(tmp, "full"), save_step=2)
    res["reducer"] = (type(full.reducer) is GradBucketReducer, full.reducer.stats["steps"])
    res["full_w"], res["full_buffer"] = full.w.detach().clone(), int(full.steps_seen)
    res["validate"] = T.validate(full, _loaders(rank, world, B_RANK, 4)[1], IT0 + 4, seed=7)
    # (b) two iterations, a checkpoint, new objects, resume, two more
    first = _Stub()
    res["part_logs"], _ = _train(T, cfg, first, _loaders(rank, world, B_RANK, 2), IT0, os.path.join(tmp, "part"), save_step=2)
    torch.manual_seed(4242 + rank)
    second = _Stub()
    with torch.no_grad():
        second.w.mul_(3)
    opt = _SGD(second, cfg.SOLVER.LR)
    loaders = _loaders(rank, world, B_RANK, 4, seed=999)
    it = T.resume(cfg, os.path.join(tmp, "part"), IT0 + 2, second, opt, loaders[0])
    res["rng_restored"] = torch.equal(torch.get_rng_state(), torch.load(os.path.join(tmp, "part", "trainer", f"iteration_{IT0 + 2}.pth"))
                                      ["ranks"][rank]["cpu_rng"])
    res["rest_logs"], _ = _train(T, cfg, second, loaders, it, None, opt=opt)
    res["resumed_w"], res["resumed_alpha"], res["full_alpha"] = second.w.detach().clone(), second.ss_loss_fn.alpha, full.ss_loss_fn.alpha
    # (c) a replica that drifted is caught before anything is written, on both ranks
    drift = _Stub()
    hooks_dir = os.path.join(tmp, "drift")
    try:
        opt = _SGD(drift, cfg.SOLVER.LR)

        def after(it_, m, rec):
            if it_ == IT0 + 1 and rank == 1:
                with torch.no_grad():
                    m.w[1] = torch.nextafter(m.w[1], m.w[1] + 1)
        T.do_train(cfg, drift, opt, T.build_scheduler(cfg, opt, IT0), _loaders(rank, world, B_RANK, 4)[0], None, resume_iter=IT0, log_step=2,
                   save_step=2, output_dir=hooks_dir, log=lambda r: None, hooks={"after_step": after})
        res["drift"] = None
    except agree.ReplicaMismatch as e:
        res["drift"] = (str(e), e.names)
    res["saves"] = saves
    out[rank] = res
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dp"))
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, _free_port(), tmp, out), nprocs=WORLD, join=True)
    return tmp, out[0], out[1]


@pytest.fixture(scope="module")
def one_process():
    """the reference: ONE process, no torch.distributed, the single loader with batch 2 b over the same dataset with the same seeds"""
    from csbsr_amd import trainer as T
    from csbsr_amd.utils import estimate_metrics as EM
    keep = EM.psnr_ssim, EM.iou_sweep
    _host_metrics()
    try:
        m = _Stub()
        logs, seen = _train(T, _cfg(), m, _loaders(0, 1, WORLD * B_RANK, 4, mode="sample"), IT0)
        val = T.validate(m, _loaders(0, 1, WORLD * B_RANK, 4, mode="sample")[1], IT0 + 4, seed=7)
    finally:
        EM.psnr_ssim, EM.iou_sweep = keep
    assert m.reducer is None
    return logs, m.w.detach().clone(), val, m.ss_loss_fn.alpha


def _close(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        if isinstance(v, float):
            assert abs(v - b[k]) <= 1e-12, (k, v, b[k])
        else:
            assert v == b[k], (k, v, b[k])


def test_logged_window_means_are_those_of_the_global_batch(two_ranks, one_process):
    _, r0, r1 = two_ranks
    logs, w, _, _ = one_process
    assert [r["iteration"] for r in logs if "segment_loss" in r] == [IT0 + 2, IT0 + 4] and len(logs) == 3
    train0 = [r for r in r0["full_logs"] if "segment_loss" in r]
    for got, want in zip(train0, [r for r in logs if "segment_loss" in r]):
        _close(got, want)
    assert len(train0) == 2 and train0[0]["segment_loss"] != train0[1]["segment_loss"]
    assert float((r0["full_w"] - w).abs().max()) <= 1e-12 and torch.equal(r0["full_w"], r1["full_w"])
    assert not torch.equal(w, _Stub().w.detach())                    # (it trained: the weights the losses depend on moved)
    assert r0["reducer"] == (True, 4) and r1["reducer"] == (True, 4)      # do_train attached it; the stub's optimiser drove it
    assert r0["full_buffer"] == r1["full_buffer"] == 4


def test_log_fires_on_rank_0_only_and_after_step_on_both(two_ranks):
    _, r0, r1 = two_ranks
    assert r1["full_logs"] == [] and r1["part_logs"] == [] and r1["rest_logs"] == []
    assert [("checkpoint" in r, "eval_sr_loss" in r, r["iteration"]) for r in r0["full_logs"]] == [
        (False, False, IT0 + 2), (True, False, IT0 + 2), (False, False, IT0 + 4), (True, False, IT0 + 4), (False, True, IT0 + 4)]
    assert r0["full_seen"] == r1["full_seen"] and [r is not None for r in r1["full_seen"]] == [False, True, False, True]
    assert r1["full_seen"][1] == r0["full_logs"][0]


def test_validation_is_that_of_one_rank_over_the_global_batches(two_ranks, one_process):
    """5 images, b = 2 on two ranks: global batches of 4 and 1, rank 1 holds nothing of the second (a None batch: no forward)"""
    _, r0, r1 = two_ranks
    logs, _, val, _ = one_process
    assert r0["validate"] == r1["validate"] and (val["batches"], val["images"]) == (2, 5)
    _close(r0["validate"], val)
    # the pass do_train ran at iteration IT0 + 4 (fresh draws, common to the ranks) against the one process's
    ev0, ev = [r for r in r0["full_logs"] if "eval_sr_loss" in r], [r for r in logs if "eval_sr_loss" in r]
    assert len(ev0) == len(ev) == 1
    _close(ev0[0], ev[0])
    # the short batch weighs as much as the full one in the losses, a fifth in the metrics: neither is a mean over images of the losses
    assert val["eval_segment_loss"] != val["eval_sr_loss"] and val["psnr"] > 0 and 0 <= val["iou"] <= 1


def test_only_rank_0_writes_and_the_file_names_the_world(two_ranks):
    tmp, r0, r1 = two_ranks
    assert r1["saves"] == []
    want = sorted(os.path.join(tmp, d, kind, f"iteration_{it}.pth") for d, its in (("full", (IT0 + 2, IT0 + 4)), ("part", (IT0 + 2, )))
                  for it in its for kind in ("model", "optimizer", "trainer"))
    assert sorted(r0["saves"]) == want and all(os.path.isfile(p) for p in want)
    st = torch.load(os.path.join(tmp, "full", "trainer", f"iteration_{IT0 + 2}.pth"))
    assert st["world"] == 2 and len(st["ranks"]) == 2 and st["iteration"] == IT0 + 2
    assert all(r["loader"] is None and r["cuda_rng"] is None and r["cpu_rng"].dtype == torch.uint8 for r in st["ranks"])       # batch mode: one common state
    assert not torch.equal(st["ranks"][0]["cpu_rng"], st["ranks"][1]["cpu_rng"])
    assert st["loader"]["global_batch"] == 4 and st["loader"]["produced"] == 2
    assert float(st["logging"]["sums"].abs().sum()) == 0                          # iteration IT0 + 2 closes a window


def test_two_plus_two_iterations_through_resume_are_four(two_ranks):
    _, r0, r1 = two_ranks
    assert r0["rng_restored"] and r1["rng_restored"]
    train = lambda logs: [r for r in logs if "segment_loss" in r]
    assert train(r0["part_logs"]) + train(r0["rest_logs"]) == train(r0["full_logs"]) and len(train(r0["full_logs"])) == 2
    assert [r for r in r0["rest_logs"] if "eval_sr_loss" in r] == [r for r in r0["full_logs"] if "eval_sr_loss" in r]
    for r in (r0, r1):
        assert torch.equal(r["resumed_w"], r["full_w"]) and r["resumed_alpha"] == r["full_alpha"]


def test_a_drifted_replica_raises_on_both_ranks_before_anything_is_written(two_ranks):
    tmp, r0, r1 = two_ranks
    assert r0["drift"] is not None and r0["drift"] == r1["drift"]
    message, names = r0["drift"]
    assert names == ["w"] and "'w'" in message and f"iteration {IT0 + 2}" in message
    assert not os.path.exists(os.path.join(tmp, "drift"))


def test_a_checkpoint_of_two_ranks_continues_on_one(two_ranks, one_process):
    """another world size with a batch-mode loader of the same global batch: everything but the generator states; a warning says so.  Any
    other change of the world size raises."""
    from csbsr_amd import trainer as T
    from csbsr_amd.utils import estimate_metrics as EM
    tmp, r0, _ = two_ranks
    logs, w, _, alpha = one_process
    cfg = _cfg()
    m = _Stub()
    opt = _SGD(m, cfg.SOLVER.LR)
    loaders = _loaders(0, 1, WORLD * B_RANK, 4, seed=31337)
    rng = torch.get_rng_state()
    with pytest.warns(UserWarning, match="2 rank"):
        it = T.resume(cfg, os.path.join(tmp, "part"), IT0 + 2, m, opt, loaders[0])
    assert torch.equal(torch.get_rng_state(), rng)
    keep = EM.psnr_ssim, EM.iou_sweep
    _host_metrics()
    try:
        rest, _ = _train(T, cfg, m, loaders, it, None, opt=opt)
    finally:
        EM.psnr_ssim, EM.iou_sweep = keep
    assert float((m.w.detach() - w).abs().max()) <= 1e-12 and m.ss_loss_fn.alpha == alpha
    for got, want in zip(rest, logs[1:]):
        _close(got, want)
    assert len(rest) == 2
    for bad in (_loaders(0, 1, WORLD * B_RANK, 4, mode="sample")[0], _loaders(0, 1, B_RANK, 4)[0], None):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(ValueError):
                T.resume(cfg, os.path.join(tmp, "part"), IT0 + 2, _Stub(), _SGD(_Stub(), 0.25), bad)
