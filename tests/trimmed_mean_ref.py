"""numpy restatement of the coordinate-wise trimmed mean's specification
(include/fedagg.h, fedagg_trimmed_mean): the reference of test_trimmed_mean.py
and test_gpu_trimmed_mean.py.  16-bit rows go through torch for the exact
widening to fp32 and for the final round-to-nearest-even narrowing."""
from __future__ import annotations

import numpy as np
import torch


def order_keys(x: np.ndarray) -> np.ndarray:
    """int32 keys of an fp32 array in the specification's total order:
    b ^ ((b >> 31) & 0x7fffffff), every NaN at 0x7fffffff (above +inf)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    k = b ^ ((b >> 31) & np.int32(0x7FFFFFFF))
    return np.where(np.isnan(x), np.int32(0x7FFFFFFF), k).astype(np.int32)


def trimmed_mean_f32(x: np.ndarray, trim: int) -> np.ndarray:
    """x: (K, N) float32.  Stable argsort on the order keys, the kept ranks
    added in ascending order as one fp32 chain starting from s[trim], an fp32
    division by the number kept."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K = x.shape[0]
    assert 0 <= trim and K - 2 * trim >= 1
    idx = np.argsort(order_keys(x), axis=0, kind="stable")
    s = np.take_along_axis(x, idx, axis=0)
    with np.errstate(all="ignore"):
        acc = s[trim].copy()
        for r in range(trim + 1, K - trim):
            acc = (acc + s[r]).astype(np.float32)
        return (acc / np.float32(K - 2 * trim)).astype(np.float32)


def trimmed_mean_ref(rows: torch.Tensor, trim: int) -> torch.Tensor:
    """rows: a (K, N) CPU tensor, fp32 / bf16 / f16 -> (N,) of the same dtype."""
    rows = rows.detach().cpu()
    out = torch.from_numpy(trimmed_mean_f32(rows.float().numpy(), trim))
    return out if rows.dtype == torch.float32 else out.to(rows.dtype)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's raw bits (int32 for fp32, int16 for 16-bit floats), on the CPU."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same(got: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """Every column: NaN where the reference is NaN, else the reference's bits."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    rn = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), rn), (what, "NaN columns differ")
    ok = rn | (bits(got) == bits(ref))
    if not bool(ok.all()):
        bad = torch.nonzero(~ok).flatten()[:5].tolist()
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ, first at {bad}: "
                             f"got {[got.flatten()[i].item() for i in bad]}, "
                             f"want {[ref.flatten()[i].item() for i in bad]}")


def trims(K: int, extra=()) -> list:
    """trim values 0, 1, (K-1)//2 and `extra`, valid for K, without repeats."""
    out = []
    for t in (0, 1, (K - 1) // 2, *extra):
        if t >= 0 and K - 2 * t >= 1 and t not in out:
            out.append(t)
    return out


def make_rows(K: int, N: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """(K, N) CPU test rows: 0.05 * randn; columns 0-15 random +-0 only;
    columns 16-31 quantised to 1/40 (ties); fp32 also gets a band of
    denormals (columns 32-47)."""
    g = torch.Generator().manual_seed(seed)
    x = 0.05 * torch.randn((K, N), generator=g)
    z = torch.zeros((K, min(N, 16)))
    z[torch.rand((K, min(N, 16)), generator=g) < 0.5] = -0.0
    x[:, :16] = z
    if N > 16:
        x[:, 16:32] = torch.round(x[:, 16:32] * 40) / 40
    if N > 32 and dtype == torch.float32:
        n = min(N, 48) - 32
        x[:, 32:48] = (torch.randn((K, n), generator=g) * 3e-39)
    return x.to(dtype)
