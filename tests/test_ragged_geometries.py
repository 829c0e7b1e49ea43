"""Ragged batches (vox_embed_lens / vox_embed_device_lens) for the two Res2Net
geometries that run on the generic kernels: res2net50_w24_s4_c64 (a 64-channel
stem on stem_conv1, layer 1 on split_chain) and res2net50_w8_s6_c16 (a
16-channel stem, every stride-1 chain on split_chain, the stride-2 branch 3x3s
on conv_igemm).  As in test_ragged.py every row of a padded batch must equal
the run of that utterance alone at its own length bit for bit, whatever the
padding holds: lengths on every residue of the x8 downsampling, the 25-frame
minimum, split_chain tiles cut by an utterance's end and tiles wholly in
padding, pools of 33 and 65 rows, NaN and large finite padding."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C64 = "res2net50_w24_s4_c64"
W8 = "res2net50_w8_s6_c16"
GEOMETRIES = [(C64, 80), (C64, 40), (W8, 40), (W8, 80)]


def _batch(lens, T, F, rng):
    """Frames first, NaN padding after."""
    x = np.full((len(lens), T, F), np.nan, np.float32)
    for i, L in enumerate(lens):
        x[i, :L] = rng.standard_normal((L, F)).astype(np.float32)
    return x


def _repad(x, lens, rng):
    """The same frames, large finite noise as padding."""
    y = x.copy()
    for i, L in enumerate(lens):
        y[i, L:] = rng.standard_normal((x.shape[1] - L, x.shape[2])) * 50
    return y


def _exact(ex, x, lens):
    """Each utterance through the ordinary path at its own length (equal
    lengths batched together: embeddings are batch-independent)."""
    out = np.empty((len(lens), ex.dim), np.float32)
    for L in sorted(set(lens)):
        idx = [i for i, l in enumerate(lens) if l == L]
        out[idx] = ex.run(np.ascontiguousarray(x[idx, :L]))
    return out


def _bad(got, exp, lens):
    return [lens[i] for i in range(len(lens)) if not np.array_equal(got[i], exp[i])]


RESIDUES = (64, [64, 63, 62, 61, 60, 59, 58, 57, 33, 26, 25])
TILES = (120, [120, 119, 113, 97, 64, 25])
CASES = [(name, F) + shape for name, F in GEOMETRIES for shape in (RESIDUES, TILES)]
CASES += [(C64, 80, 264, [264, 263, 257, 201, 129]),      # pools of 33 rows at C = 2048
          (C64, 80, 520, [520, 519, 513, 400, 263])]      # pools of 65 rows


@pytest.mark.parametrize("name,F,T,lens", CASES)
def test_rows_equal_their_exact_runs(weights, name, F, T, lens):
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(name, F)
    rng = np.random.default_rng(T + F)
    x = _batch(lens, T, F, rng)
    with Extractor(blob, precision="bf16") as ex:
        assert ex.supports_lengths()
        got = ex.run_lens(x, lens)
        exp = _exact(ex, x, lens)
        assert np.isfinite(got).all()
        bad = _bad(got, exp, lens)
        assert not bad, f"lengths {bad} differ from their exact runs"
        # the padding's values are ignored
        x2 = _repad(x, lens, np.random.default_rng(T + F + 1))
        assert np.array_equal(ex.run_lens(x2, lens), got)


def test_device_entry_replays_plan(weights):
    """run_device_lens on a side stream into fixed buffers, three rounds of
    fresh lengths on one handle: the later rounds replay the plan (and its
    captured graph), no rebuild."""
    import torch
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(C64, 80)
    rng = np.random.default_rng(5)
    T, n = 304, 32
    dev = torch.device("cuda", 0)
    with Extractor(blob, precision="bf16") as ex:
        s = torch.cuda.Stream(dev)
        xd = torch.empty((n, T, 80), dtype=torch.float32, device=dev)
        ld = torch.empty((n,), dtype=torch.int32, device=dev)
        out = torch.empty((n, ex.dim), dtype=torch.float32, device=dev)
        built = []
        for rep in range(3):
            lens = [int(v) for v in rng.integers(25, T + 1, size=n)]
            lens[0] = T
            x = _batch(lens, T, 80, rng)
            xd.copy_(torch.from_numpy(x))
            ld.copy_(torch.tensor(lens, dtype=torch.int32))
            torch.cuda.synchronize(dev)
            before = ex.plan_stats()["built"]
            ex.run_device_lens(xd, ld, out=out, stream=s)
            s.synchronize()
            built.append(ex.plan_stats()["built"] - before)
            got = out.cpu().numpy()
            bad = _bad(got, _exact(ex, x, lens), lens)
            assert not bad, (rep, bad)
        assert built == [1, 0, 0], built


@pytest.mark.parametrize("name,F", GEOMETRIES)
def test_plans_accepted_at_extractor_shapes(weights, name, F):
    """The kernel choice depends on the batch's pixel count while
    supports_lengths probes (2, 64) only: the shapes the streaming extractor
    builds must be accepted too."""
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(name, F)
    rng = np.random.default_rng(F)
    with Extractor(blob, precision="bf16") as ex:
        for n, T in ((1, 25), (1, 1000), (64, 200), (16, 1000)):
            lens = [int(v) for v in rng.integers(25, T + 1, size=n)]
            lens[0] = T
            x = rng.standard_normal((n, T, F)).astype(np.float32)
            out = ex.run_lens(x, lens)            # raises VoxError where a plan refuses
            assert np.isfinite(out).all(), (n, T)


def _write_fm_ark(path, mats):
    """Binary FM ark as kaldi_io.write_mat writes it; returns scp lines."""
    import struct
    lines = []
    with open(path, "wb") as f:
        for key, m in mats:
            f.write(key.encode() + b" ")
            off = f.tell()
            f.write(b"\0BFM \x04" + struct.pack("<i", m.shape[0]) + b"\x04" +
                    struct.pack("<i", m.shape[1]) + m.astype("<f4").tobytes())
            lines.append(f"{key} {path}:{off}\n")
    return lines


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name,F", [(C64, 80), (W8, 40)])
def test_stream_takes_ragged_path(weights, tmp_path, name, F, lanes):
    """stream.extract_entries with ragged=None picks the ragged path by itself;
    lengths across the 1000-frame chunk boundary, batches of 3, same bits as
    the chunk loop through one handle's host API."""
    from voxsrc2020_speaker_verification_amd import extract, kaldi
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    from voxsrc2020_speaker_verification_amd.stream import extract_entries
    spec, t, blob = weights(name, F)
    rng = np.random.default_rng(11)
    lens = [30, 1030, 999, 1000, 1001, 25, 180, 180, 260]
    mats = [(f"u{i:02d}", (rng.standard_normal((T, F)) * 2 + 1).astype(np.float32))
            for i, T in enumerate(lens)]
    scp = _write_fm_ark(str(tmp_path / "f.ark"), mats)
    (tmp_path / "f.scp").write_text("".join(scp))
    entries = kaldi.read_scp(str(tmp_path / "f.scp"))
    exs = [Extractor(blob, device=0, precision="bf16") for _ in range(lanes)]
    try:
        assert exs[0].supports_lengths()
        keys, got = extract_entries(entries, exs, batch=3, ragged=None)
    finally:
        for e in exs:
            e.close()
    with Extractor(blob, device=0, precision="bf16") as ex:
        feats = list(kaldi.iter_features(str(tmp_path / "f.scp")))
        ref = extract.embed_utterances(feats, ex.run, ex.dim, 3)
    assert keys == [k for k, _ in mats]
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("name,precision", [("dpn68", "bf16"), (C64, "fp32")])
def test_still_refused(weights, name, precision):
    from voxsrc2020_speaker_verification_amd._native import VoxError
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(name, 80)
    x = np.zeros((2, 64, 80), np.float32)
    with Extractor(blob, precision=precision) as ex:
        assert not ex.supports_lengths()
        with pytest.raises(VoxError):
            ex.run_lens(x, [64, 40])
        ex.run(x)                                   # the handle still works
