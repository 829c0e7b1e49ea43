"""The attentive-pooling tail kernel (attpool.hip att_pool_k) on its own,
through vox_debug_att_pool: softmax over time of the logits, weighted mean and
std of x (models.py:273-303), with per-utterance lengths (ragged batches).

Shapes keep n*w*c no multiple of the 256 threads of a block, three below it and
one between one and two blocks: a block spans utterances (the row count is per
thread) and the tail block is partly empty.  Row counts sit on both sides of
the 32 rows the kernel keeps in
registers (h = 40: 40 / 33 / 13 rows; h = 70: 70 / 65 / 33 / 32).

Accuracy bar: the stats-pool kernel's (test_stats_pool_kernel: rtol = atol =
1e-5 at unit-scale inputs) against a float64 statement of the pooling, for the
launch without lengths.  The masked launches need no tolerance: they are
bitwise equal to unmasked launches."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 1e-5

# (n, h, w, c) -> (lengths at vsh = 3, the valid rows ceil(len / 8) they give)
SHAPES = {
    (5, 9, 3, 16): ([72, 65, 64, 33, 25], [9, 9, 8, 5, 4]),
    (3, 40, 2, 24): ([320, 257, 100], [40, 33, 13]),
    (4, 70, 1, 8): ([560, 520, 264, 256], [70, 65, 33, 32]),
    # n*w*c = 360: a full block whose threads span utterances, then a partly empty one
    (3, 12, 5, 24): ([96, 50, 25], [12, 7, 4]),
}
_DATA = {}


def _data(shape, dtype):
    """(x, logits) device tensors ~ N(0, 1), made once per (shape, dtype) and
    never written to."""
    import torch
    key = (shape, dtype)
    if key not in _DATA:
        rng = np.random.default_rng(sum(shape))
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to("cuda")
        x = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32).contiguous()
        lg = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to("cuda")
        _DATA[key] = (x, lg)
    return _DATA[key]


def _pool(x, lg, lens=None, vsh=0):
    """One launch; x [n,h,w,c] bf16 / fp32, lg fp32, lens a python list or None."""
    import torch
    from voxsrc2020_speaker_verification_amd import _native
    n, h, w, c = x.shape
    assert x.is_contiguous() and lg.is_contiguous() and lg.dtype == torch.float32
    assert lg.shape == x.shape
    code = _native.VOX_BF16 if x.dtype == torch.bfloat16 else _native.VOX_FP32
    ld = None
    if lens is not None:
        assert len(lens) == n
        ld = torch.tensor(lens, dtype=torch.int32, device=x.device)
    out = torch.full((n, w * 2 * c), float("nan"), dtype=torch.float32, device=x.device)
    _native.check(_native.lib().vox_debug_att_pool(
        C.c_void_p(x.data_ptr()), C.c_void_p(lg.data_ptr()),
        C.c_void_p(ld.data_ptr()) if ld is not None else None, vsh, n, h, w, c, code, EPS,
        C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _alone(x, lg, rows):
    """Every utterance launched on its own at h = its valid rows, no lengths."""
    return np.concatenate([_pool(x[i:i + 1, :r].contiguous(), lg[i:i + 1, :r].contiguous())
                           for i, r in enumerate(rows)])


def _padded(x, lg, rows, xfill, lfill):
    x2, lg2 = x.clone(), lg.clone()
    for i, r in enumerate(rows):
        x2[i, r:] = xfill
        lg2[i, r:] = lfill
    return x2, lg2


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_att_pool_matches_float64(shape, dtype):
    """No lengths: the weighted mean / std against float64 numpy, at the
    stats-pool kernel's bar."""
    x, lg = _data(shape, dtype)
    got = _pool(x, lg)
    xr = x.float().cpu().numpy().astype(np.float64)
    l = lg.cpu().numpy().astype(np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    wt = e / e.sum(axis=1, keepdims=True)
    wm = (xr * wt).sum(axis=1)                                   # [n, w, c]
    sd = np.sqrt((xr * xr * wt).sum(axis=1) - wm * wm + EPS)
    ref = np.concatenate([wm, sd], axis=2).reshape(shape[0], -1)  # feature w*2c + {c | C + c}
    err = np.abs(got - ref).max()
    print(f"att_pool {shape} {dtype}: max abs err {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("vsh", [3, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_att_pool_lengths_bitwise(shape, vsh, dtype):
    """A padded utterance with Hn valid rows gives the bits of an h = Hn launch
    on it alone, whatever the padding holds (NaN, +-1e30: the rows at or past
    Hn are never read)."""
    x, lg = _data(shape, dtype)
    lens3, rows = SHAPES[shape]
    lens = lens3 if vsh == 3 else rows
    exp = _alone(x, lg, rows)
    assert np.isfinite(exp).all()
    got = _pool(x, lg, lens, vsh)
    bad = [i for i in range(len(rows)) if not np.array_equal(_bits(got[i]), _bits(exp[i]))]
    assert not bad, f"utterances {bad} (rows {[rows[i] for i in bad]}) differ from their own launches"
    for xfill, lfill in ((float("nan"), float("nan")), (1e30, 1e30), (-1e30, -1e30),
                         (1e30, -1e30)):
        x2, lg2 = _padded(x, lg, rows, xfill, lfill)
        assert np.array_equal(_bits(_pool(x2, lg2, lens, vsh)), _bits(got)), (xfill, lfill)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_att_pool_full_lengths_equal_no_lengths(shape, dtype):
    x, lg = _data(shape, dtype)
    n, h = shape[:2]
    plain = _pool(x, lg)
    assert np.array_equal(_bits(_pool(x, lg, [h * 8] * n, 3)), _bits(plain))
    assert np.array_equal(_bits(_pool(x, lg, [h * 8 - 7] * n, 3)), _bits(plain))
    assert np.array_equal(_bits(_pool(x, lg, [h] * n, 0)), _bits(plain))
    # a length past the batch's rows is clamped to them
    assert np.array_equal(_bits(_pool(x, lg, [h + 5] * n, 0)), _bits(plain))
