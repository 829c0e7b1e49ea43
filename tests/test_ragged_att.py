"""Ragged batches through the attentive-pooling Res2Nets
(res2net101_w24_s4_c32_att, bf16): the backbone masks padded rows as the
res2net50 plan's does (tests/test_ragged.py); the attention tail's two pools
take each utterance's own rows (attpool.hip, stats_pool_k RAG) and everything
between them is per pixel.  Every row of a ragged batch must equal the run of
that utterance alone at its own length, bit for bit, whatever the padding
holds."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "res2net101_w24_s4_c32_att"


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


@pytest.mark.parametrize("F", [80, 40])
def test_att_supports_lengths(weights, F):
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(MODEL, F)
    with Extractor(blob, precision="bf16") as ex:
        assert ex.supports_lengths()


@pytest.mark.parametrize("F,T,lens", [
    # every residue of the x8 downsampling, the 25-frame minimum
    (80, 120, [120, 119, 118, 117, 116, 115, 114, 113, 97, 64, 33, 25]),
    (80, 264, [264, 263, 257, 256, 201, 129]),          # pools of 33 rows
    (80, 520, [520, 513, 512, 505, 263]),               # pools of >= 64 rows
    (40, 120, [120, 119, 113, 97, 64, 25]),
])
def test_ragged_att_bitwise_equal_exact_runs(weights, F, T, lens):
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(MODEL, F)
    rng = np.random.default_rng(T + F)
    x = _batch(lens, T, F, rng)
    with Extractor(blob, precision="bf16") as ex:
        got = ex.run_lens(x, lens)
        exp = _exact(ex, x, lens)
        assert np.isfinite(got).all()
        bad = _bad(got, exp, lens)
        assert not bad, f"lengths {bad} differ from their exact runs"
        # the padding's values are ignored
        x2 = _repad(x, lens, np.random.default_rng(T + F + 1))
        assert np.array_equal(ex.run_lens(x2, lens), got)


def test_ragged_att_full_lengths_equal_plain_run(weights):
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(MODEL, 80)
    x = np.random.default_rng(3).standard_normal((4, 120, 80)).astype(np.float32)
    with Extractor(blob, precision="bf16") as ex:
        assert np.array_equal(ex.run_lens(x, [120] * 4), ex.run(x))


def test_ragged_att_device_entry_replays_plan(weights):
    """run_device_lens on a side stream, three times with fresh lengths on one
    handle: the later calls replay the plan (and its captured graph) with new
    lengths, no rebuild."""
    import torch
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(MODEL, 80)
    rng = np.random.default_rng(5)
    T, n = 160, 12
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
def test_stream_att_takes_ragged_path(weights, tmp_path, lanes):
    """stream.extract_entries with ragged=None picks the ragged path by itself
    for the attentive-pooling model; lengths across the 1000-frame chunk
    boundary, batches of 3, same bits as the chunk loop through one handle's
    host API."""
    from voxsrc2020_speaker_verification_amd import extract, kaldi
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    from voxsrc2020_speaker_verification_amd.stream import extract_entries
    spec, t, blob = weights(MODEL, 80)
    rng = np.random.default_rng(11)
    lens = [30, 1030, 999, 1000, 1001, 25, 180, 180, 260]
    mats = [(f"u{i:02d}", (rng.standard_normal((T, 80)) * 2 + 1).astype(np.float32))
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


def test_att_fp32_still_refuses_lengths(weights):
    from voxsrc2020_speaker_verification_amd._native import VoxError
    from voxsrc2020_speaker_verification_amd.extractor import Extractor
    spec, t, blob = weights(MODEL, 80)
    x = np.zeros((2, 64, 80), np.float32)
    with Extractor(blob, precision="fp32") as ex:
        assert not ex.supports_lengths()
        with pytest.raises(VoxError):
            ex.run_lens(x, [64, 40])
        ex.run(x)                                   # the handle still works
