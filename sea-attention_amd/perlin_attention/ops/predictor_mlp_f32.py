"""The predictor MLP for fp32 data in one launch (include/sea_hip_predictor_mlp_f32.h, csrc/sea_mlp_f32.hip).

`predictor_mlp_f32(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin)` is `ops.predictor_mlp` for fp32 tensors: encoder Linear + LayerNorm +
GELU, the row decoder's Linear, ChannelSplit(2) + cnn.lnorm1 stored in the C8 layout of the convolutions, and the two sigmoid gates,
every product on the fp32 matrix instruction.  Nothing is rounded to 16 bit."""
import torch

from ... import _lib
from .flat_csr import _p
from .predictor import _cached


def predictor_mlp_f32_supported(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin) -> bool:
    """What the kernel takes (one predicate on both sides of the ABI, `sea_predictor_mlp_f32_supported`): a device tensor x
    (N, H, T, Din) of fp32 with a contiguous last axis and 16-byte aligned rows, affine modules with biases, and a (D1, D2, H, Din)
    the library has a form for (d = 64: D1 = 128, Din = 192; D2 in {16, 32, 48, 64, 128}; H % 4 == 0)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
        return False
    N, H, T, Din = x.shape
    if min(N, H, T, Din) < 1 or N * H * T >= (1 << 31) - 64 or x.stride(-1) != 1 or any(s % 4 for s in x.stride()[:3]) or x.data_ptr() % 16:
        return False
    if any(m.bias is None for m in (enc_lin, dec_lin, scaler_lin)) or not (enc_ln.elementwise_affine and ln1.elementwise_affine):
        return False
    D1, D2 = enc_lin.out_features, dec_lin.out_features
    if (enc_lin.in_features != Din or dec_lin.in_features != D1 or tuple(enc_ln.normalized_shape) != (D1,)
            or tuple(ln1.normalized_shape) != (D2 // 2,) or scaler_lin.in_features != D1 or scaler_lin.out_features != 2):
        return False
    return bool(_lib.load().sea_predictor_mlp_f32_supported(D1, D2, H, Din))


def _pack_f32_fragments(w: torch.Tensor) -> torch.Tensor:
    """(M, K) weight -> MFMA 16x16x4 A fragments in blocks of four k-steps, [M/16][K/16][64 lanes][4]: lane 16 g + i of fragment
    (tile, kb) holds W[16 tile + i][16 kb + 4 g + j], j = 0 .. 3 (step j of the block multiplies the k set {16 kb + 4 g + j : g})."""
    M, K = w.shape
    return w.reshape(M // 16, 16, K // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


def mlp_f32_images(device, enc_lin, enc_ln, dec_lin, ln1, scaler_lin):
    """(w1_packed, w2_packed, vectors) of csrc/sea_mlp_f32.hip for these modules, cached per parameter set (`_cached`)."""
    def build():
        f = lambda t: t.detach().to(device=device, dtype=torch.float32)
        vec = torch.cat([f(t).reshape(-1) for t in (enc_lin.bias, enc_ln.weight, enc_ln.bias, dec_lin.bias, ln1.weight, ln1.bias,
                                                    scaler_lin.weight, scaler_lin.bias)]).contiguous()
        return _pack_f32_fragments(f(enc_lin.weight)), _pack_f32_fragments(f(dec_lin.weight)), vec
    return _cached("mlp_f32", (enc_lin.weight, enc_lin.bias, enc_ln.weight, enc_ln.bias, dec_lin.weight, dec_lin.bias,
                               ln1.weight, ln1.bias, scaler_lin.weight, scaler_lin.bias), torch.float32, build)


@_lib.device_guarded
def predictor_mlp_f32(x: torch.Tensor, enc_lin, enc_ln, dec_lin, ln1, scaler_lin, want_tpred: bool = False):
    """x (N, H, T, Din) fp32 -> (x_c8 (N, T, H*2/8, Wd, 8), tpred (N, H, T, D1) or None, row_scale (N, H, T), avg_scale (N, H, T)), all
    fp32.  Raises where `predictor_mlp_f32_supported` does not hold: there is no other path behind this name."""
    if not predictor_mlp_f32_supported(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin):
        raise RuntimeError(f"predictor_mlp_f32: x {tuple(x.shape) if isinstance(x, torch.Tensor) else x} {getattr(x, 'dtype', None)}, "
                           f"D1={enc_lin.out_features}, D2={dec_lin.out_features} is outside the fp32 kernel "
                           "(ops.predictor_mlp_f32_supported)")
    lib = _lib.load()
    N, H, T, Din = x.shape
    D1, D2 = enc_lin.out_features, dec_lin.out_features
    w1p, w2p, vec = mlp_f32_images(x.device, enc_lin, enc_ln, dec_lin, ln1, scaler_lin)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    x_c8, row_scale, avg_scale = f32(N, T, H * 2 // 8, D2 // 2, 8), f32(N, H, T), f32(N, H, T)
    tpred = f32(N, H, T, D1) if want_tpred else None
    _lib.check(lib.sea_predictor_mlp_f32(_p(x), N, H, T, Din, _lib.strides3(x), D1, D2, _p(w1p), _p(w2p), _p(vec), float(enc_ln.eps),
                                         float(ln1.eps), _p(x_c8), 0, _p(tpred), _p(row_scale), _p(avg_scale), _lib.stream_ptr()),
               "sea_predictor_mlp_f32")
    return x_c8, tpred, row_scale, avg_scale
