"""The weight-stationary form of the 16-bit convolution (`causal_conv_ring_kernel`, sea_conv.hip) against the kernel it stands in
for: the library is built a second time with the form compiled out (-DSEA_CONV_NO_RING), both builds run the same launches in
child processes (SEA_HIP_LIB), and every output must be the same bytes.  The new form keeps the MFMA, the operand placement,
the k order and the epilogue, so nothing less than bit identity is expected (the decode tests rely on that order)."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, dtype, N, T, dil, relu, one_hot).  Launches of >= 32768 rows take the new form on a 256-CU part (128 rows per CU);
# the 8192-row ones stay on the register form and pin the routing itself.
CASES = []
for dt in ("bf16", "f16"):
    for dil in (1, 2, 3):
        CASES.append((f"x8_{dt}_d{dil}", dt, 8, 4096, dil, 1, False))
        CASES.append((f"ragged_{dt}_d{dil}_relu", dt, 9, 3701, dil, 1, False))      # 33309 rows: not a multiple of 4 x CUs
        CASES.append((f"ragged_{dt}_d{dil}_lin", dt, 9, 3701, dil, 0, False))
    CASES.append((f"x1_{dt}_d2_relu", dt, 1, 8192, 2, 1, False))
    CASES.append((f"x1_{dt}_d2_lin", dt, 1, 8192, 2, 0, False))
    CASES.append((f"short6_{dt}_d3", dt, 5500, 6, 3, 1, False))                      # T <= 2 dil: every row in the causal padding
    CASES.append((f"short3_{dt}_d2", dt, 11000, 3, 2, 0, False))
    CASES.append((f"short2_{dt}_d1", dt, 16500, 2, 1, 1, False))
CASES += [("x8_bf16_d2_lin", "bf16", 8, 4096, 2, 0, False), ("x1_bf16_d1", "bf16", 1, 8192, 1, 1, False),
          ("x1_bf16_d3", "bf16", 1, 8192, 3, 0, False), ("onehot_bf16_d2", "bf16", 8, 4096, 2, 0, True),
          ("onehot_f16_d1", "f16", 8, 4096, 1, 0, True)]


def _child(out_path):
    """Run every case with the library SEA_HIP_LIB names; write {case: sha256 of the output's bytes}."""
    sys.path.insert(0, ROOT)
    import torch
    from sea_attention_amd.perlin_attention import ops
    dev = "cuda"
    C, W = 64, 64
    res = {}
    for name, dt, N, T, dil, relu, one_hot in CASES:
        dtype = torch.bfloat16 if dt == "bf16" else torch.float16
        g = torch.Generator(device=dev).manual_seed(zlib.crc32(name.encode()))
        if one_hot:
            x = torch.zeros((N, C, T, W), device=dev)
            x[1, 37, 100, 0] = 1.0                                       # first pixel of a row: the left taps' edge
            x[2, 5, 7, 63] = 1.0                                         # last pixel, inside the causal ramp
            x[0, 63, 4095, 31] = 1.0
        else:
            x = torch.relu(torch.randn((N, C, T, W), device=dev, generator=g))
        x = ops.to_c8(x.to(dtype))
        wt = (torch.randn((C, C, 5, 3), device=dev, generator=g) * (C * 9) ** -0.5).to(dtype)
        b = (torch.randn(C, device=dev, generator=g) * 0.1).to(dtype)
        y = ops.causal_conv_c8(x, wt, b, 3, dil, dil, relu=bool(relu))
        torch.cuda.synchronize()
        assert y.is_contiguous()
        res[name] = hashlib.sha256(y.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
        del x, y
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.mark.gpu
def test_ring_form_equals_the_register_form_bit_for_bit(tmp_path):
    from sea_attention_amd import _build
    ring_lib = _build.ensure_built()
    plain_lib = _build.build_library(extra_flags=("-DSEA_CONV_NO_RING",), out=str(tmp_path / "libsea_hip_noring.so"))
    outs = {}
    for tag, lib in (("ring", ring_lib), ("plain", plain_lib)):
        out = tmp_path / f"{tag}.json"
        env = dict(os.environ, SEA_HIP_LIB=lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, f"{tag}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        outs[tag] = json.loads(out.read_text())
    assert set(outs["ring"]) == {c[0] for c in CASES}
    bad = [k for k in outs["ring"] if outs["ring"][k] != outs["plain"][k]]
    assert not bad, f"outputs differ between the two forms: {bad}"


if __name__ == "__main__":
    _child(sys.argv[1])
