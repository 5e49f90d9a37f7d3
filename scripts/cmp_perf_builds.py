#!/usr/bin/env python3
"""Bit comparison of the 16-bit Performer kernels of two builds of the library.

    python scripts/cmp_perf_builds.py <other libsea_hip.so>      (e.g. the parent commit's, `_build.build_library(out=...)`)

Every case runs in a fresh child process per library (the tree's own, and the other one through SEA_HIP_LIB) and prints
whether `out`, `avg` and the state image of the two are byte-equal.  Cases: bf16 and fp16 x the five kernel forms, N = 1,
H = 2, T = 200 (a ragged last chunk at both chunk sizes; two segments fit): `performer_value` with 1 and 2 segments and
`want_avg`, then `performer_step` fed 70 rows, 70 single rows (device position, image updated in place: most of these steps
close no chunk and write nothing) and the rest.  Exit status 1 when anything differs."""
import math
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = [(64, 33, "D = 64, NBT = 3"), (64, 66, "D = 64, NBT = 5"), (80, 43, "D = 80, NBT = 3"), (80, 58, "D = 80, NBT = 5"),
         (128, 77, "D = 128, NBT = 5")]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
N, H, T = 1, 2, 200


def run_case(D, nb, dtype, path):
    from sea_attention_amd.perlin_attention import ops
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(1000 * D + nb)
    rnd = lambda *s: torch.randn(s, generator=g)
    q = (rnd(N, H, T, D) * D ** -0.5).to(dev, dtype)
    k, v, pos = rnd(N, H, T, D).to(dev, dtype), rnd(N, H, T, D).to(dev, dtype), rnd(T, D).to(dev, dtype)
    proj = (rnd(nb, D) * math.sqrt(D) / 4).to(dev)
    res = {}
    for nseg in (1, 2):
        res[f"value{nseg}.out"], res[f"value{nseg}.avg"] = ops.performer_value(q, k, v, pos, proj, want_avg=True, n_segments=nseg)
    outs, avgs = [], []
    o, a, state = ops.performer_step(q[:, :, :70], k, v, pos, proj, None, 0)
    outs.append(o), avgs.append(a)
    res["step.state70"] = state.clone()
    seen = torch.zeros((1,), dtype=torch.int32, device=dev)
    for t in range(70, 140):                                   # one row at a time, the position in device memory
        seen.fill_(t)
        o, a, state = ops.performer_step(q[:, :, t:t + 1], k, v, pos, proj, state, 0, t_base_dev=seen)
        outs.append(o), avgs.append(a)
    res["step.state140"] = state.clone()
    o, a, state = ops.performer_step(q[:, :, 140:], k, v, pos, proj, state, 140)
    outs.append(o), avgs.append(a)
    res["step.out"], res["step.avg"], res["step.state"] = torch.cat(outs, 2), torch.cat(avgs, 2), state
    torch.cuda.synchronize()
    torch.save({n: t.cpu().contiguous().view(torch.uint8) for n, t in res.items()}, path)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--case":
        return run_case(int(sys.argv[2]), int(sys.argv[3]), DTYPES[sys.argv[4].split(":")[0]], sys.argv[4].split(":", 1)[1])
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    other = os.path.abspath(sys.argv[1])
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for dname in DTYPES:
            for D, nb, form in FORMS:
                got = []
                for tag, lib in (("tree", None), ("other", other)):
                    env = {k_: v_ for k_, v_ in os.environ.items() if k_ != "SEA_HIP_LIB"}
                    if lib:
                        env["SEA_HIP_LIB"] = lib
                    path = os.path.join(tmp, f"{tag}.pt")
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(D), str(nb), f"{dname}:{path}"],
                                   env=env, check=True, timeout=300)
                    got.append(torch.load(path))
                diff = [n for n in got[0] if not torch.equal(got[0][n], got[1][n])]
                bad += bool(diff)
                print(f"{dname} {form} (nb = {nb}): " + ("byte-equal" if not diff else "DIFFERENT in " + ", ".join(diff)) +
                      f"  [{len(got[0])} tensors]", flush=True)
    print("all byte-equal" if not bad else f"{bad} case(s) differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
