"""Data-parallel training on the device: csbsr_fingerprint against its numpy restatement (tests/fingerprint_cases.py), the batch-mode
loader's tensors against the single loader's, and do_train over two ranks on one device (gloo, as tests/test_data_parallel_gpu.py runs
them: RCCL refuses two ranks per GPU) with the replica check passing on a clean run and raising on both ranks for a one-ulp drift."""
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fingerprint_cases as FC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.fixture(scope="module")
def fp_list():
    """(names, device tensors, host arrays): fingerprint_cases.host_cases plus two views that start 4 bytes into their allocations (the
    word-by-word path: one of less than a chunk, one of more than two)"""
    cases = FC.host_cases()
    rng = np.random.default_rng(9)
    holds = []
    for n in (5, 20001):
        whole = rng.integers(0, 2 ** 32, size=n + 1, dtype=np.uint64).astype("<u4").view(np.float32)
        holds.append((f"unaligned_{n}", whole))
    names = [n for n, _ in cases] + [n for n, _ in holds]
    dev = [torch.from_numpy(a).to(DEV) for _, a in cases] + [torch.from_numpy(a).to(DEV)[1:] for _, a in holds]
    host = [a for _, a in cases] + [a[1:] for _, a in holds]
    assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in dev[-2:]) and dev[names.index("empty")].numel() == 0
    assert {t.dtype for t in dev} == {torch.float32, torch.int64}
    for t, a in zip(dev, host):          # the upload kept every bit (NaN payloads included)
        assert np.array_equal(FC.words_of(t.cpu().numpy()), FC.words_of(a))
    return names, dev, host


def test_fingerprint_equals_the_numpy_restatement_bit_for_bit(fp_list):
    from csbsr_amd.parallel import agree
    names, dev, host = fp_list
    want = torch.from_numpy(FC.fingerprint_numpy(host))
    got = agree.fingerprint(dev)
    again = agree.fingerprint(dev)
    assert got.dtype == torch.int64 and got.shape == (len(dev), 2) and got.device == dev[0].device
    for i, n in enumerate(names):
        print(f"  {n}: device {got[i].tolist()} numpy {want[i].tolist()}")
    for i, n in enumerate(names):
        assert torch.equal(got[i].cpu(), want[i]), n
    assert torch.equal(got, again)
    assert got[names.index("empty")].tolist() == [0, 0]
    # another launch geometry for the same words: one tensor alone, and the list reversed
    k = names.index("f32_20000")
    assert torch.equal(agree.fingerprint([dev[k]])[0], got[k])
    assert torch.equal(agree.fingerprint(dev[::-1]), got.flip(0))


def test_fingerprint_table_staging_reuse_and_growth(fp_list):
    """The pinned table of agree.fingerprint through its life: allocated for 3 rows (72 B in the 4096 B minimum), reused for 40 rows
    (960 B) and for the first 3 again, then outgrown by 180 rows (4320 B).  Every table is the numpy restatement, bit for bit."""
    from csbsr_amd.parallel import agree
    _, dev, host = fp_list
    agree._host.pop(DEV, None)          # whatever earlier tests left: the sequence starts from no staging
    rng = np.random.default_rng(13)
    ones = [rng.integers(0, 2 ** 32, size=1, dtype=np.uint64).astype("<u4").view(np.float32) for _ in range(180)]
    pick = [i % len(dev) for i in range(40)]
    lists = [(dev[:3], host[:3]), ([dev[i] for i in pick], [host[i] for i in pick]), (dev[:3], host[:3]),
             ([torch.from_numpy(a).to(DEV) for a in ones], ones)]
    got = [agree.fingerprint(d) for d, _ in lists]
    for k, (g, (_, h)) in enumerate(zip(got, lists)):
        assert torch.equal(g.cpu(), torch.from_numpy(FC.fingerprint_numpy(h))), f"call {k}"


def test_fingerprint_sees_a_flipped_bit_and_an_exchange(fp_list):
    from csbsr_amd.parallel import agree
    names, dev, _ = fp_list
    dev = [t.clone() for t in dev]
    base = agree.fingerprint(dev)
    k = names.index("f32_8193")
    words = dev[k].view(torch.int32)
    words[8192] ^= 1 << 22                                   # one bit of the one element in the second chunk
    flipped = agree.fingerprint(dev)
    others = [i for i in range(len(dev)) if i != k]
    assert torch.equal(flipped[others], base[others])
    assert flipped[k, 0] != base[k, 0] and flipped[k, 1] != base[k, 1]
    assert abs(int(flipped[k, 0]) - int(base[k, 0])) == 1 << 22
    words[8192] ^= 1 << 22
    assert torch.equal(agree.fingerprint(dev), base)
    # an exchange of two unequal words, one in each chunk: the plain sum cannot see it, the weighted sum must
    a, b = int(words[17]), int(words[8192])
    assert a != b
    words[17], words[8192] = b, a
    swapped = agree.fingerprint(dev)
    assert torch.equal(swapped[others], base[others])
    assert swapped[k, 0] == base[k, 0] and swapped[k, 1] != base[k, 1]
    # int64 tensors: an exchange of two ELEMENTS moves both of their words
    k = names.index("i64_10000")
    e = dev[k]
    x, y = int(e[3]), int(e[9000])
    e[3], e[9000] = y, x
    swapped = agree.fingerprint(dev)
    assert swapped[k, 0] == base[k, 0] and swapped[k, 1] != base[k, 1]


def test_replicas_agree_in_one_process_and_refusals_on_the_device(fp_list):
    from csbsr_amd.parallel import agree
    names, dev, _ = fp_list
    assert agree.replicas_agree(list(zip(names, dev))) == []          # one replica: nothing to differ from
    agree.assert_replicas_agree(dict(zip(names, dev)))
    with pytest.raises(ValueError):
        agree.fingerprint([torch.zeros(4, 6, device=DEV)[:, ::2]])
    with pytest.raises(ValueError):
        agree.fingerprint([torch.zeros(6, dtype=torch.float16, device=DEV)[:5]])
    with pytest.raises(ValueError):
        agree.fingerprint([dev[0], torch.zeros(3, dtype=torch.uint8, device=DEV)])
    from csbsr_amd import _lib as L
    with pytest.raises(L.CsbsrHipError):
        agree.fingerprint([dev[0], torch.zeros(4)])               # one of the list on the host


# ----------------------------------------------------------------------------------------------------------------- 2. the loader
def _pool(n=6, size=64):
    from csbsr_amd.data.resident import ResidentDataset
    rng = np.random.default_rng(7)
    images, masks = [], []
    for _ in range(n):
        yy, xx = np.mgrid[0:size, 0:size]
        base = 128 + 60 * np.sin(xx / rng.uniform(4, 9) + rng.uniform(0, 3)) * np.cos(yy / rng.uniform(4, 9))
        img = np.clip(base[:, :, None] + rng.normal(0, 12, size=(size, size, 3)), 0, 255).astype(np.uint8)
        m = np.zeros((size, size), np.uint8)
        c = (xx * rng.uniform(0.3, 0.9) + rng.uniform(5, 25)).astype(int)
        m[np.abs(yy - c) < 2] = 255
        img[m > 0] //= 3
        images.append(img)
        masks.append(m)
    return ResidentDataset(images, masks, device=DEV)


@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized_crop"])
def test_batch_mode_tensors_are_the_rows_of_the_single_loaders(resized):
    from csbsr_amd.data.resident import DeviceTrainLoader
    ds = _pool()
    kw = dict(seed=13, drop_last=True, num_iterations=3, vflip_p=0.3, resized_crop={"scale": (0.3, 1.0), "ratio": (0.75, 1.25)} if resized else None)
    single = DeviceTrainLoader(ds, 32, 4, batch_size=4, **kw)
    ranks = [DeviceTrainLoader(ds, 32, 4, batch_size=2, shard=(r, 2), shard_mode="batch", **kw) for r in range(2)]
    steps = 0
    for whole, a, b in zip(single, *ranks):
        assert len(whole) == len(a) == len(b) == 5
        for i, (w, x, y) in enumerate(zip(whole, a, b)):
            assert x.shape[0] == y.shape[0] == 2 and w.shape[0] == 4
            assert torch.equal(w[:2], x) and torch.equal(w[2:], y), (steps, i)
        steps += 1
    assert steps == 3 and ranks[0].produced == ranks[1].produced == single.produced == 3
    assert float(whole[1].std()) > 0.01


# ----------------------------------------------------------------------------------------------------------------- 3. two ranks
IT0 = 39999          # a multiple of save_step = 3: iterations IT0 + 1 .. IT0 + 3 end with the checkpoint, as iterations 1 .. 3 would


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _small_cfg():
    from csbsr_amd.config import cfg as base_cfg
    cfg = base_cfg.clone()
    cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE, cfg.MODEL.OPTIMIZER = 4, "PSPNet", "Adam"
    cfg.SOLVER.BATCH_SIZE = 2
    cfg.SOLVER.SR_PRETRAIN_ITER = [1, IT0 - 1]          # the run (IT0 + 1 ..) is in the joint phase: every parameter trains
    return cfg


def _small_model(cfg):
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModelWithLoss(cfg, 6, IT0, None, device=DEV)
    deterministic_fill(m.state_dict(), "contractive")
    m.micro_batch, m.max_resident = 1, 8          # two micro-batches per rank, as in tests/test_data_parallel_gpu.py
    return m


def _worker(rank, world, port, tmp, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader
    from csbsr_amd.parallel import agree
    torch.cuda.set_device(0)
    cfg = _small_cfg()
    ds = _pool()
    res = {}

    import time
    t0 = time.time()
    torch.manual_seed(5 + rank)                               # Dropout2d's masks are per replica
    m = _small_model(cfg)
    if rank == 1:                                             # the replicas start apart: the broadcast makes them one
        with torch.no_grad():
            next(m.parameters()).add_(1.0)
    opt = T.build_optimizer(cfg, m)
    res["t_build"] = time.time() - t0

    def run(name, it0, hooks=None):
        """three iterations from it0 + 1, the checkpoint at the third"""
        t0 = time.time()
        ld = DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=3, seed=31 + it0, drop_last=True, shard=(rank, world), shard_mode="batch")
        logs = []
        try:
            T.do_train(cfg, m, opt, T.build_scheduler(cfg, opt, it0), ld, resume_iter=it0, log_step=1, save_step=3,
                       output_dir=os.path.join(tmp, name), log=logs.append, hooks=hooks)
        finally:
            torch.cuda.synchronize()
            res["t_" + name] = time.time() - t0
        return logs

    logs = run("clean", IT0)
    res["logs"] = [(r["iteration"], r["segment_loss"], r["sr_loss"]) for r in logs if "segment_loss" in r]
    res["reducer"] = dict(m.reducer.stats)
    # what differs between the replicas after three steps, running statistics included (every rank gets the same list)
    res["differ_all"] = agree.replicas_agree(T.replica_tensors(m, opt))
    res["checked"] = len(T.replica_tensors(m, opt, running_stats=False))
    target = next(k for k, v in m._named_full() if isinstance(v, torch.nn.Parameter) and k.startswith("sr_model") and v.numel() > 8)
    res["target"] = target

    def after(it, model, rec):
        if it == IT0 + 5 and rank == 1:                       # the second of the next three iterations
            p = dict(model._named_full())[target].data.view(-1)
            p[3] = torch.nextafter(p[3], p[3] + 1)            # one ulp, one element, one rank
    try:                                                      # the same replicas go on (do_train broadcasts and checks them again)
        run("drift", IT0 + 3, {"after_step": after})
        res["drift"] = None
    except agree.ReplicaMismatch as e:
        res["drift"] = (str(e), list(e.names))
    out[rank] = res
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dp_gpu"))
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), tmp, out), nprocs=2, join=True)
    return tmp, out[0], out[1]


def test_two_ranks_train_check_and_rank_0_writes(two_ranks):
    tmp, r0, r1 = two_ranks
    print("  seconds per rank: " + ", ".join(f"{k[2:]} {r0[k]:.1f} / {r1[k]:.1f}" for k in ("t_build", "t_clean", "t_drift")))
    assert [r[0] for r in r0["logs"]] == [IT0 + 1, IT0 + 2, IT0 + 3] and r1["logs"] == []
    assert all(np.isfinite(r[1]) and np.isfinite(r[2]) for r in r0["logs"])
    for kind in ("model", "optimizer", "trainer"):
        assert os.listdir(os.path.join(tmp, "clean", kind)) == [f"iteration_{IT0 + 3}.pth"]
    st = torch.load(os.path.join(tmp, "clean", "trainer", f"iteration_{IT0 + 3}.pth"))
    assert st["world"] == 2 and len(st["ranks"]) == 2 and all(r["cuda_rng"] is not None and r["loader"] is None for r in st["ranks"])
    assert st["loader"]["global_batch"] == 4 and st["loader"]["produced"] == 3
    # the reducer do_train attached exchanged the six buckets of every step under the backward
    for r in (r0, r1):
        assert r["reducer"]["steps"] == 3 and r["reducer"]["all_reduces"] == 18 and r["reducer"]["on_side_stream"] == 18, r["reducer"]
    # the check covered every parameter, the batch counters and both Adam moments; all that differs between the replicas is what is per
    # replica by design: BatchNorm's running statistics
    assert r0["checked"] == r1["checked"] and r0["checked"] >= 3 * 290
    assert r0["differ_all"] == r1["differ_all"]
    print(f"  {r0['checked']} tensors checked at the checkpoint; {len(r0['differ_all'])} running statistics differ between the replicas")
    assert all(n.endswith((".running_mean", ".running_var")) for n in r0["differ_all"]), r0["differ_all"][:5]


def test_one_ulp_on_one_rank_raises_on_both_and_nothing_is_written(two_ranks):
    tmp, r0, r1 = two_ranks
    assert r0["drift"] is not None and r1["drift"] is not None and r0["drift"] == r1["drift"]
    message, names = r0["drift"]
    print("  ", message)
    assert names[0] == r0["target"] and repr(r0["target"]) in message and f"iteration {IT0 + 6}" in message
    assert not os.path.exists(os.path.join(tmp, "drift"))
