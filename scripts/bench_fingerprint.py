"""Rate of the replica fingerprint (csbsr_fingerprint, csbsr_amd/parallel/agree.py) over the model's parameter set.

    python scripts/bench_fingerprint.py --out profiles/fingerprint_bench.json

One leg, in a child process under its own time limit (the parent never opens the GPU): ``agree.fingerprint`` over every parameter and
buffer of the KBPN + PSPNet model (one launch, 4 bytes read per word), next to ``csbsr_amd.optim.SGD.step()`` over the same parameters in
the same run (20 bytes per element) as the yardstick of what this chunk map reaches.  Wall clock between two synchronisations, >= 50
calls per window, two windows, the better one reported.  No criterion is attached: the fingerprint runs once per checkpoint.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
LEG_TIMEOUT_S = 300


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def leg(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.optim import SGD
    from csbsr_amd.parallel import agree
    model = JointModelWithLoss(base_cfg.clone(), 9000, 0, None, device=DEV)
    tensors = [t.detach().to(DEV).clone() for t in model.state_dict().values()]
    params = [torch.nn.Parameter(p.detach().to(DEV).clone()) for p in model.parameters()]
    gen = torch.Generator(device=DEV).manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
    sgd = SGD(params, lr=2e-5, momentum=0.9, weight_decay=5e-4)
    nbytes = sum(t.numel() * t.element_size() for t in tensors)
    n = sum(p.numel() for p in params)
    first = agree.fingerprint(tensors)
    for _ in range(a.warmup):
        agree.fingerprint(tensors)
        sgd.step()
    fp = min(wall_ms(lambda: agree.fingerprint(tensors), a.steps) for _ in range(2))
    st = min(wall_ms(sgd.step, a.steps) for _ in range(2))
    return {"bench": "fingerprint", "tensors": len(tensors), "bytes": nbytes, "steps": a.steps, "fingerprint_ms": round(fp, 4),
            "fingerprint_gb_per_s": round(nbytes / fp / 1e6, 1), "sgd_elements": n, "sgd_ms": round(st, 4),
            "sgd_gb_per_s": round(20 * n / st / 1e6, 1), "same_table_every_call": bool(torch.equal(first, agree.fingerprint(tensors)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true", help="run the leg in this process (default: in a child process)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps must be at least 50")
    if a.leg:
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(leg(a)), flush=True)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        print(f"no result within {LEG_TIMEOUT_S} s", file=sys.stderr)
        sys.exit(124)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        sys.exit(r.returncode if r.returncode > 0 else 1)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
