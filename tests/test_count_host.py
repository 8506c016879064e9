"""Triangle counts on the host: tests/count_cases.py's scenes N(n) -- n on and next to 8, 64, 256,
512, 4 096, 8 192, 32 768, 65 536 and 131 072, sentinels at the tails of the spatial order, and the
dead-tail variants -- through the CPU backend and the host restatements (query_host, layers_host,
attributes_host), against the oracle. No GPU.

The case guards run here with the oracle's answers: a change of the construction that hides a
sentinel, or moves one off its order position, fails in test_guards. The CPU backend bins by screen
box in blocks of its own, so the count edges matter to it too; ids exact, RGB within 1e-5
(test_gpu_parity.assert_parity). A frame that differs only on the device is a device bug
(test_gpu_count.py).
"""
from __future__ import annotations

import numpy as np
import pytest

import count_cases as cc
import gbuffer_cases as gc
import layers_cases as lc
import query_cases as qc
import simpleraytracer_amd as srt
import simpleraytracer_amd.device as device
from test_gpu_parity import assert_parity

POINT_NAMES = cc.SMALL_NAMES + cc.DEAD_NAMES


@pytest.fixture
def cpu(monkeypatch):
    monkeypatch.setenv("ML_VISIBLE_DEVICES", "cpu")
    monkeypatch.setenv("SRT_CPU_THREADS", "4")


def test_sentinel_positions():
    """The order positions asked for, where they exist."""
    assert cc.sentinel_positions(1, 1) == [0]
    assert cc.sentinel_positions(9, 9) == [0, 1, 7, 8]
    assert cc.sentinel_positions(513, 513) == [0, 1, 7, 8, 255, 256, 257, 504, 505, 511, 512]
    assert cc.sentinel_positions(4096, 4096) == [0, 1, 7, 8, 255, 256, 3839, 3840, 4087, 4088, 4094, 4095]
    assert cc.sentinel_positions(256, 257) == [0, 1, 7, 8, 247, 248, 249, 254, 255]
    assert [cc.id_planes(n) for n in cc.PLANE_COUNTS] == [0, 1, 1, 1, 2]


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_guards(name):
    """The sentinels sit at the tails of the restated order (asserted in case()); each wins a pixel of
    the oracle's frame, ids 0 and n - 1 among them; the hit share; no dead id wins, and the dead ids
    are the order's tail (frame()); every sentinel is the layer-0 answer at a position (answers(),
    layers())."""
    c = cc.case(name)
    n, dead = cc.parse(name)
    assert (c.n, c.dead, len(c.order)) == (n, dead, n)
    assert np.array_equal(np.sort(c.order), np.arange(n))
    assert [int(c.order[p]) for p in c.positions] == list(c.sentinels[:len(c.positions)])
    assert {0, c.live - 1} <= set(c.sentinels)
    won = set(np.unique(cc.frame_ids(name)).tolist())
    assert set(c.sentinels) <= won and -1 in won
    assert not any(i >= c.live for i in won)
    if dead:
        assert set(c.order[c.live:].tolist()) == set(range(c.live, n))
    _, ids, _ = cc.layers(name)
    assert set(c.sentinels) <= set(ids[0].tolist())


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_cpu_backend_equals_oracle(cpu, name):
    c = cc.case(name)
    for kind in ("rnd", "half"):
        got = srt.render(c.path, cc.W, cc.H, cc.offsets(cc.W, cc.H, kind))
        assert_parity(got, cc.frame(name, kind))


@pytest.mark.parametrize("name", cc.SMALL_NAMES + cc.DEAD_NAMES)
def test_cpu_backend_odd_frame(cpu, name):
    """200 x 72: a partial last tile column and row."""
    c = cc.case(name)
    got = srt.render(c.path, cc.ODD_W, cc.ODD_H, cc.offsets(cc.ODD_W, cc.ODD_H))
    assert_parity(got, cc.frame(name, "rnd", cc.ODD_W, cc.ODD_H))


@pytest.mark.parametrize("name", POINT_NAMES)
def test_query_and_layers_host(name):
    """Exact against the oracle at the mixed positions, the sentinels' centroids and a pixel each wins."""
    c = cc.case(name)
    pos, want_ids, want_t = cc.answers(name)
    ids, t = device.query_host(c.path, cc.W, cc.H, pos)
    qc.assert_same(ids, t, want_ids, want_t)
    _, l_ids, l_t = cc.layers(name)
    ids4, t4 = device.layers_host(c.path, cc.W, cc.H, pos, cc.LAYERS)
    lc.assert_same(ids4, t4, l_ids, l_t)


@pytest.mark.parametrize("name", POINT_NAMES)
def test_attributes_host(name):
    """Every plane against the oracle and numpy (gbuffer_cases): id n - 1 reads the last entry."""
    c = cc.case(name)
    pos, ids, t = cc.answers(name)
    assert c.live - 1 in ids
    exp = gc.expected(c.path, cc.W, cc.H, pos, ids)
    depth, bary, normal, albedo = device.attributes_host(c.path, cc.W, cc.H, pos, ids)
    gc.check_planes(exp, depth, bary, normal, albedo)
    gc.check_misses(ids, exp.n, exp.background, depth, bary, normal, albedo)
    assert np.array_equal(depth.view(np.uint32), t.view(np.uint32))  # the oracle's full scan
