"""python -m kgvae.experiments.interpolation over a checkpoint written by kgvae.experiments.train (synthetic syn-paths-shaped
data, as tests/test_models_gpu.py::test_train_entry_point_end_to_end): the four analyses run for every epsilon of the
reference's list, each on one per-latent decode call."""
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu


def test_interpolation_entry_point_over_a_train_checkpoint(tmp_path, capsys, monkeypatch):
    from kgvae.experiments import interpolation as I
    from kgvae.experiments import train as T
    from kgvae.model.models import SAIL
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "sail_syn-paths.yaml")))
    cfg.update(model_type="SAIL", d_model=64, num_epochs=2, batch_size=64, save_every=2, compression_log_every=2,
               learning_rate=1e-3, synthetic_sizes={"n_train": 512, "n_val": 128, "n_test": 64})
    cpath = tmp_path / "c.yaml"
    yaml.safe_dump(cfg, open(cpath, "w"))
    T.main(["--config", str(cpath), "--checkpoint-dir", str(tmp_path / "ck")])
    run = tmp_path / "ck" / os.listdir(tmp_path / "ck")[0]
    calls = []
    inner = SAIL.decode_latent

    def spy(self, z, *a, **kw):
        calls.append((z.shape[0], kw.get("beam"), kw.get("per_latent", False)))
        return inner(self, z, *a, **kw)

    monkeypatch.setattr(SAIL, "decode_latent", spy)
    capsys.readouterr()
    torch.manual_seed(0)
    assert I.main(["--config", str(cpath), "--checkpoint-dir", str(run), "--directions", "5"]) == 0
    out = capsys.readouterr().out
    n = len(I.EPSILONS)
    assert I.EPSILONS == [0.02, 0.05, 0.07, 0.1, 0.12, 0.15, 0.17, 0.2]
    for mark in ("=== Local Latent Neighborhood Exploration ===", "=== Latent Smoothness Line Walk ===", "[SMOOTHNESS SCORE]",
                 "[FLIP RATE]"):
        assert out.count(mark) == n, mark
    beam = cfg.get("beam_width", 3)
    per_eps = [(1, 3, True), (5, 3, True), (11, beam, True), (3 * 3 * 11, beam, True), (5 * 4 * 31, beam, True)]
    assert calls == per_eps * n
