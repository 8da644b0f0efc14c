"""The persistent list kernel's primary-ray batches (kernels.hip k_render, PRIM).

In the chunked analytic list kernel (samples_per_unit < spp, no mesh, no world BVH, no extended
features: the cornell box) a wave traces primary rays 64 at a time, one sample of its unit's 8x8
block, in iterations of their own; the lanes that hold a path park it in LDS for that iteration
and the lanes left without a hit take the parked paths back. Every draw is keyed by (pixel,
sample, phase) and every sample has its own scratch slot, so only the order of work changes: each
frame here is BITWISE the CPU restatement's (the oracle), as in test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
import yart

pytestmark = pytest.mark.gpu

DEPTH = 50


@pytest.fixture(scope="module")
def cornell():
    p = yart.Preset("cornell-box")
    return p, yart.DeviceScene(p)


@pytest.fixture(scope="module")
def ref_44x20():
    """The oracle's cornell-box 44x20 frames, shared by the cases that render that size."""
    p = yart.Preset("cornell-box")
    cam = p.camera(44, 20)
    o = O.OracleScene(p.desc)
    return {spp: o.render(cam, yart.render_params(44, 20, spp, DEPTH)) for spp in (4, 6)}


@pytest.mark.parametrize("spu", [1, 2, 5])
def test_partial_blocks_and_short_last_units(cornell, ref_44x20, spu):
    """44 is not a multiple of 8: the batches of the right-hand blocks have dead slots. 5 does not
    divide 6 spp: the last unit of each block is short, and parked paths cross unit boundaries."""
    p, s = cornell
    W, H, spp = 44, 20, 6
    got = s.render(p.camera(W, H), yart.render_params(W, H, spp, DEPTH, samples_per_unit=spu))
    np.testing.assert_array_equal(got, ref_44x20[spp])
    cov = O.coverage(W, H)
    assert (got[~cov] == 0).all() and (got[cov].sum(axis=-1) != 0).mean() > 0.05


@pytest.mark.parametrize("max_depth", [0, 1, 2])
def test_depth_edges(cornell, max_depth):
    """max_depth 0: every sample ends inside its batch (reflectance 1), nothing is ever parked or
    scattered. 1: every path ends at its first scatter or before. 2: one world pass after it."""
    p, s = cornell
    W, H, spp = 24, 16, 3
    cam = p.camera(W, H)
    got = s.render(cam, yart.render_params(W, H, spp, max_depth, samples_per_unit=1))
    np.testing.assert_array_equal(got, O.OracleScene(p.desc).render(cam, yart.render_params(W, H, spp, max_depth)))
    assert (got[O.coverage(W, H)].sum(axis=-1) != 0).mean() > 0.05


def test_primary_rays_that_mostly_end_in_the_batch():
    """The cornell box with every object but the light and the floor removed: most primary rays
    miss (black background) or hit the emitter and end inside their batch, so one hand-out runs
    several batches before the lanes that asked have a path."""
    p = yart.Preset("cornell-box")
    d = p.desc.contents
    keep = [2, 3]  # the flipped light rect and the floor (host/presets.cpp cornell_box)
    kept = (type(d.objects[0]) * len(keep))(*[d.objects[i] for i in keep])
    d.objects = C.cast(kept, type(d.objects))
    d.n_objects = len(keep)
    W, H, spp = 40, 24, 4
    cam = p.camera(W, H)
    got = yart.DeviceScene(p.desc).render(cam, yart.render_params(W, H, spp, DEPTH, samples_per_unit=1))
    ref = O.OracleScene(p.desc).render(cam, yart.render_params(W, H, spp, DEPTH))
    np.testing.assert_array_equal(got, ref)
    cov = O.coverage(W, H)
    lit = (ref[cov].sum(axis=-1) != 0).mean()
    assert 0.02 < lit < 0.9, lit  # some paths go on from the floor, many samples end black


def test_shards_and_a_packed_shard(cornell, ref_44x20):
    """Shards 0..2 of 3 sum to the oracle's frame; shard 1 once more through the block-packed path."""
    p, s = cornell
    W, H, spp, n = 44, 20, 4, 3
    cam = p.camera(W, H)
    ref = ref_44x20[spp]
    parts = [s.render(cam, yart.render_params(W, H, spp, DEPTH, shard_index=k, shard_count=n, samples_per_unit=1))
             for k in range(n)]
    np.testing.assert_array_equal(parts[0] + parts[1] + parts[2], ref)
    k = 1
    d = torch.zeros(yart.shard_packed_len(W, H, k, n), dtype=torch.float64, device="cuda:0")
    st = torch.cuda.current_stream()
    s.render_packed_async(cam, yart.render_params(W, H, spp, DEPTH, shard_index=k, shard_count=n, samples_per_unit=1),
                          d.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    pk = d.cpu().numpy().reshape(-1, 64, 3)
    cov = O.coverage(W, H)
    bx = (W + 7) // 8
    seen = 0
    for j in range(pk.shape[0]):
        b = k + j * n
        for slot in range(64):
            x, y = (b % bx) * 8 + slot % 8, (b // bx) * 8 + slot // 8
            if x < W and y < H and cov[y, x]:
                np.testing.assert_array_equal(pk[j, slot], ref[y, x])
                seen += 1
    assert seen > 0


def test_two_frames_back_to_back_on_each_of_two_streams(cornell):
    """The benchmark's pattern: frames alternate over two streams, so a frame's persistent waves
    start beside the previous frame's last long paths. Each frame equals its single render."""
    p, s = cornell
    W, H, spp = 40, 24, 8
    cams = [yart.make_camera((278.0 + 30.0 * k, 278.0, -800.0), (278.0, 278.0 - 20.0 * k, 0.0), 40.0, W / H, 0.0)
            for k in range(4)]
    prm = yart.render_params(W, H, spp, DEPTH, samples_per_unit=1)
    single = [s.render(c, prm) for c in cams]
    sts = [torch.cuda.current_stream(), torch.cuda.Stream()]
    outs = [torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda:0") for _ in cams]
    torch.cuda.synchronize()
    for k, (c, out) in enumerate(zip(cams, outs)):
        st = sts[k % 2]
        with torch.cuda.stream(st):
            s.render_async(c, prm, out.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    for k, (out, ref) in enumerate(zip(outs, single)):
        np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"frame {k}")
    np.testing.assert_array_equal(single[0], O.OracleScene(p.desc).render(cams[0], yart.render_params(W, H, spp, DEPTH)))


def test_counters_match_the_fused_kernel(cornell):
    """The algorithmic counters do not depend on the order of work: the persistent kernel
    (samples_per_unit = 1, primary rays in batches) counts what the fused kernel
    (samples_per_unit = spp, one unit per block, untouched by the batches) counts. The lane
    counters differ by design: camera_iters counts batches, camera_lanes their lanes.
    All four equalities hold on the kernels before the batches too."""
    p, s = cornell
    W, H, spp = 40, 24, 8
    cam = p.camera(W, H)
    _, per = s.render_with_stats(cam, yart.render_params(W, H, spp, DEPTH, samples_per_unit=1))
    _, fused = s.render_with_stats(cam, yart.render_params(W, H, spp, DEPTH, samples_per_unit=spp))
    covered = int(O.coverage(W, H).sum())
    assert per.samples == covered * spp == fused.samples
    assert per.segments == fused.segments and per.segments > per.samples
    assert per.prim_tests == fused.prim_tests and per.prim_tests > 0
    assert per.light_tests == fused.light_tests and per.light_tests > 0
    # every sample starts in a batch; a batch holds at most one sample of each of a block's pixels
    assert per.camera_lanes == per.samples
    blocks = ((W + 7) // 8) * ((H + 7) // 8)
    assert blocks * spp >= per.camera_iters >= -(-per.samples // 64)
