"""fresco_amd.propagate's host logic (no GPU): the lockstep schedule over unequal intervals, grouping by packed layout
and weights, max_batch cuts, the composed argv and the output / .bin paths; the batch cap against the header."""
import os
import re
import sys

import numpy as np
import pytest

from fresco_amd import ebsynth as E
from fresco_amd import propagate as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import video_blend_standins as S  # noqa: E402


def chains_of(tmp_path, key_ind):
    vs = S.VideoSequence(str(tmp_path), key_ind)
    return [P.Chain(vs, i, fwd) for i in range(vs.n_seq) for fwd in (True, False)]


def test_lockstep_schedule_over_unequal_intervals(tmp_path):
    chains = chains_of(tmp_path, [0, 2, 7, 10])  # intervals 2, 5, 3
    assert [c.interval for c in chains] == [2, 2, 5, 5, 3, 3]
    assert P.steps(chains) == [(1, [0, 1, 2, 3, 4, 5]), (2, [2, 3, 4, 5]), (3, [2, 3]), (4, [2, 3])]
    # every in-between frame of every chain exactly once, in its own order
    frames = [(k, j) for j, live in P.steps(chains) for k in live]
    assert sorted(frames) == sorted((k, j) for k, c in enumerate(chains) for j in range(1, c.interval))
    assert P.steps([]) == []


def test_chain_paths_and_argv(tmp_path):
    base = str(tmp_path)
    fwd, bwd = chains_of(tmp_path, [0, 3])
    assert fwd.key_img == os.path.join(base, "keys", "0000.png") and bwd.key_img == os.path.join(base, "keys",
                                                                                                   "0003.png")
    assert fwd.outputs == [os.path.join(base, "out_0", "%04d.jpg" % k) for k in (0, 1, 2)]
    assert bwd.outputs == [os.path.join(base, "out_3", "%04d.jpg" % k) for k in (3, 2, 1)]
    a = fwd.argv(2)
    t = os.path.join(base, "tmp", "out_0")
    assert a == ["-style", fwd.key_img,
                 "-guide", fwd.inputs[0], fwd.inputs[2], "-weight", "6",
                 "-guide", os.path.join(t, "edge_0000.jpg"), os.path.join(t, "edge_0002.jpg"), "-weight", "0.5",
                 "-guide", os.path.join(t, "temporal_0000.jpg"), os.path.join(t, "temporal_0002.jpg"), "-weight",
                 "0.5",
                 "-guide", os.path.join(t, "pos_0000.jpg"), os.path.join(t, "pos_0002.jpg"), "-weight", "2",
                 "-output", fwd.outputs[2], "-searchvoteiters", "12", "-patchmatchiters", "6"]
    cfg = E.parse_cli(a)
    assert [g[2] for g in cfg["guides"]] == [6.0, 0.5, 0.5, 2.0]
    assert cfg["searchvoteiters"] == 12 and cfg["patchmatchiters"] == 6 and cfg["output"] == fwd.outputs[2]
    assert E.bin_path(cfg["output"]) == os.path.join(base, "out_0", "0002.bin")
    cmd = P.compose_cmd(fwd.key_img, fwd.guide_pairs(2), fwd.outputs[2], "./ebsynth")
    assert cmd.split()[0] == "./ebsynth" and cmd.split()[1:] == a


def job(shape=(8, 8), ns=3, ng=12, sw=None, gw=None, **cfg):
    c = dict(uniformity=3500.0, patchsize=5, pyramidlevels=-1, searchvoteiters=12, patchmatchiters=6,
             stopthreshold=5, extrapass3x3=False)
    c.update(cfg)
    return dict(cfg=c, style=np.zeros(shape + (ns,), np.uint8), source_guide=np.zeros(shape + (ng,), np.uint8),
                target_guide=np.zeros(shape + (ng,), np.uint8), style_weights=sw or [1.0 / ns] * ns,
                guide_weights=gw or [0.5] * ng)


def test_grouping_and_max_batch_cuts():
    jobs = [job(), job(), job(ns=1), job(), job(gw=[0.25] * 12), job(), job(shape=(8, 9)), job(searchvoteiters=6),
            job()]
    assert P.batches(jobs, 2) == [[0, 1], [3, 5], [8], [2], [4], [6], [7]]
    assert P.batches(jobs, 1) == [[k] for k in (0, 1, 3, 5, 8, 2, 4, 6, 7)]
    assert P.batches(jobs, None) == [[0, 1, 3, 5, 8], [2], [4], [6], [7]]
    assert P.batches(jobs, 1000) == P.batches(jobs, E.MAX_BATCH)
    many = [job() for _ in range(E.MAX_BATCH + 5)]
    assert [len(b) for b in P.batches(many, None)] == [E.MAX_BATCH, 5]
    assert P.batches([], 3) == []


def test_default_max_batch_follows_workspace():
    big = job(shape=(2048, 2048))
    one = E.batch_workspace_bytes(1, 3, 12, (2048, 2048), (2048, 2048))
    assert P.default_max_batch(big) == max(1, min(E.MAX_BATCH, P.WORKSPACE_BUDGET // one)) < E.MAX_BATCH
    assert P.default_max_batch(job(shape=(64, 64))) == E.MAX_BATCH
    assert E.batch_workspace_bytes(3, 3, 12, (40, 40), (40, 40)) > 2 * E.batch_workspace_bytes(1, 3, 12, (40, 40),
                                                                                                 (40, 40))


def test_batch_cap_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "fresco_hip.h")).read()
    assert int(re.search(r"#define FRESCO_EBSYNTH_MAX_BATCH (\d+)", hdr).group(1)) == E.MAX_BATCH


def test_first_positional_image():
    img = P.first_positional_image(5, 7)
    assert img.dtype == np.float64 and img.shape == (5, 7, 3)
    assert (img[..., 0] == 0).all()
    np.testing.assert_array_equal(img[:, 0, 2], [0, 63, 127, 191, 255])
    np.testing.assert_array_equal(img[0, :, 1], (np.linspace(0, 1, 7) * 255).astype(np.uint8))


def test_load_job_packs_like_the_shim(tmp_path):
    base = str(tmp_path)
    S.make_video(base, [0, 3])
    vs = S.VideoSequence(base, [0, 3])
    c = P.Chain(vs, 0, True)
    for seq in (c.edges, c.temporal, c.pos):
        for p, f in zip(seq, c.inputs):
            S.imwrite(p, S.imread(f))
    j = P.load_job(c.argv(1))
    assert j["style"].shape == (24, 28, 3) and j["source_guide"].shape == (24, 28, 12)
    np.testing.assert_array_equal(j["style"], E._load_rgba(c.key_img)[..., :3])
    assert j["guide_weights"] == [float(np.float32(w) / np.float32(3)) for w in (6, 0.5, 0.5, 2) for _ in range(3)]
    with pytest.raises(E.CliError):
        P.load_job(c.argv(1)[:-4] + ["-weight"])
