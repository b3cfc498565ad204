"""bench.dump_outputs on host tensors: the sampled form of the dump (outputs longer than the kept
sizes) is a fixed, seeded, sorted sample, the same from call to call, within the size bound."""
import os

import numpy as np

import bench


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import torch
    # the 64 MB bound on a dump, with the real sizes
    assert bench.DUMP_IDS * 4 + bench.DUMP_OFFS * 8 + 8 <= 64 * 1000 * 1000
    monkeypatch.setattr(bench, "DUMP_IDS", 1000)
    monkeypatch.setattr(bench, "DUMP_OFFS", 500)
    rng = np.random.default_rng(7)
    ntok, n_docs = 50_000, 4_000
    ids = torch.from_numpy(rng.integers(0, 50_257, size=ntok + 100).astype(np.int32))  # (capacity past ntok)
    tok_off = torch.from_numpy(np.concatenate([[0], np.sort(rng.integers(0, ntok, size=n_docs - 1)), [ntok]]).astype(np.int64))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, 0, ids, tok_off, ntok)
    bench.dump_outputs(b, 0, ids, tok_off, ntok)
    assert sorted(os.listdir(a)) == ["ids_sample.npy", "n_tokens.npy", "tok_off_sample.npy"]
    for name in os.listdir(a):
        assert np.array_equal(np.load(os.path.join(a, name)), np.load(os.path.join(b, name))), name
    got_ids = np.load(os.path.join(a, "ids_sample.npy"))
    got_off = np.load(os.path.join(a, "tok_off_sample.npy"))
    assert got_ids.dtype == np.float32 and got_ids.shape == (1000,)
    assert got_off.dtype == np.float64 and got_off.shape == (500,)
    assert np.load(os.path.join(a, "n_tokens.npy")).tolist() == [float(ntok)]
    # the positions: the generator dump_outputs documents, ids first, then the offsets
    g = np.random.default_rng([0x44554D50, 0])
    pos = np.sort(g.integers(0, ntok, size=1000))
    docs = np.sort(g.integers(0, n_docs + 1, size=500))
    assert np.array_equal(got_ids, ids.numpy()[pos].astype(np.float32))
    assert np.array_equal(got_off, tok_off.numpy()[docs].astype(np.float64))
    # another rank writes its own names
    bench.dump_outputs(a, 3, ids, tok_off, ntok)
    assert "ids_sample_rank3.npy" in os.listdir(a)
