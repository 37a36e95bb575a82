"""The keypoint section of the multi-GPU result packet (runner.ResultGatherer
keyps_k / keyps_rows) on CPU tensors: keyps_k = 0 leaves the packet as it was, the
keypoint model's packet (with_masks=False, keyps_k=17) round-trips, rows past
keyps_rows travel through finish(keyps_full=), and a world-2 gloo gather delivers
every rank's rows bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

K = 17


def _rank_outputs(rank, F=3, D=16, counts=None):
    """Per-rank keypoint-model outputs; keyps frame-major like the engine's."""
    rng = np.random.default_rng(300 + rank)
    counts = np.asarray(counts if counts is not None else rng.integers(0, D + 1, F), np.int32)
    dets = np.zeros((F, D, 5), np.float32)
    cls = np.zeros((F, D), np.int32)
    for f in range(F):
        dets[f, :counts[f]] = rng.uniform(0, 100, (counts[f], 5))
        cls[f, :counts[f]] = 1
    keyps = rng.uniform(-5, 500, (int(counts.sum()), 4, K)).astype(np.float32)
    return dets, cls, counts, keyps


def _t(arrs):
    return [torch.from_numpy(a) for a in arrs]


def test_keyps_k_zero_is_todays_packet():
    from vosdetectron_amd.runner import ResultGatherer
    F, D, R = 3, 16, 28
    for kw in (dict(mask_rows=48), dict(with_masks=False)):
        g = ResultGatherer(F, D, R, 1, "cpu", **kw)
        g0 = ResultGatherer(F, D, R, 1, "cpu", keyps_k=0, keyps_rows=77, **kw)
        rows = 48 if g.with_masks else 0
        assert g.L == g0.L == F * D * 5 + F * D + F + rows * R * R
        assert (g0.o_cls, g0.o_cnt, g0.o_msk, g0.o_kps) == (F * D * 5, F * D * 6, F * D * 6 + F,
                                                            g.L)
        assert g0.keyps_rows == 0 and g0.bytes_per_rank == 4 * g.L
        dets, cls, counts, _ = _rank_outputs(0)
        masks = torch.rand(int(counts.sum()), R, R)
        a = g.gather(*_t((dets, cls, counts)), masks)
        b = g0.gather(*_t((dets, cls, counts)), masks)
        assert set(a) == set(b) and "keyps" not in b and "keyps_offsets" not in b
        assert torch.equal(g.send[0], g0.send[0])  # the packet, word for word
        for k in a:
            assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="masks is required"):
        ResultGatherer(F, D, R, 1, "cpu").gather_async(*_t((dets, cls, counts)))


def test_keypoint_packet_round_trip():
    from vosdetectron_amd.runner import ResultGatherer, frame_keyps
    F, D = 3, 16
    dets, cls, counts, keyps = _rank_outputs(1, counts=[5, 0, 11])
    g = ResultGatherer(F, D, 28, 1, "cpu", with_masks=False, keyps_k=K)
    assert g.keyps_rows == F * 100 and g.mask_rows == 0
    assert g.L == F * D * 6 + F + g.keyps_rows * 4 * K and g.o_kps == g.o_msk
    v = g.gather(*_t((dets, cls, counts)), keyps=torch.from_numpy(keyps))
    assert "masks" not in v and tuple(v["keyps"].shape) == (1, 300, 4, K)
    assert np.array_equal(v["dets"].numpy(), dets) and np.array_equal(v["counts"].numpy(), counts)
    assert v["keyps_offsets"].tolist() == [[0, 5, 5]]
    assert np.array_equal(v["keyps"][0, :16].numpy(), keyps) and not v["keyps"][0, 16:].any()
    o = 0
    for f in range(F):
        got = frame_keyps(v, F, f)
        assert tuple(got.shape) == (counts[f], 4, K)
        assert np.array_equal(got.numpy(), keyps[o:o + counts[f]])
        o += counts[f]
    # masks and keypoints side by side: each section at its own offset
    both = ResultGatherer(F, D, 4, 1, "cpu", mask_rows=20, keyps_k=K, keyps_rows=20)
    assert both.o_kps == both.o_msk + 20 * 16 and both.L == both.o_kps + 20 * 4 * K
    masks = torch.rand(16, 4, 4)
    w = both.gather(*_t((dets, cls, counts)), masks, keyps=torch.from_numpy(keyps))
    assert torch.equal(w["masks"][0, :16], masks)
    assert np.array_equal(w["keyps"][0, :16].numpy(), keyps)
    # a failed frame's negative count holds no rows
    bad = counts.copy()
    bad[1] = -1
    vb = g.gather(*_t((dets, cls, bad)), keyps=torch.from_numpy(keyps))
    assert vb["keyps_offsets"].tolist() == [[0, 5, 5]] and frame_keyps(vb, F, 1).shape[0] == 0
    with pytest.raises(ValueError, match="keyps must be M x 4 x 17"):
        g.gather_async(*_t((dets, cls, counts)), keyps=torch.zeros(16, 4, 16))
    with pytest.raises(ValueError, match="keyps must be M x 4 x 17"):
        g.gather_async(*_t((dets, cls, counts)))


def test_keyps_overflow_single_process():
    from vosdetectron_amd.runner import ResultGatherer, frame_keyps
    F, D = 3, 16
    dets, cls, counts, keyps = _rank_outputs(1, counts=[5, 16, 11])
    t = _t((dets, cls, counts))
    kt = torch.from_numpy(keyps)
    g = ResultGatherer(F, D, 28, 1, "cpu", with_masks=False, keyps_k=K, keyps_rows=10)
    v = g.gather_async(*t, keyps=kt).wait(clone=True)
    assert np.array_equal(frame_keyps(v, F, 0).numpy(), keyps[:5])
    with pytest.raises(RuntimeError, match="keypoints"):
        frame_keyps(v, F, 1)
    fin = g.gather_async(*t, keyps=kt).finish()
    assert tuple(fin["keyps_extra"].shape) == (1, 22, 4, K) and "masks_extra" not in fin
    o = 0
    for f in range(F):
        assert np.array_equal(frame_keyps(fin, F, f).numpy(), keyps[o:o + counts[f]])
        o += counts[f]
    # the engine path: the packet had only keyps_rows rows, complete() added the rest
    fin2 = g.gather_async(*t, keyps=kt[:10]).finish(keyps_full=kt)
    assert torch.equal(fin2["keyps_extra"][0], kt[10:])
    with pytest.raises(RuntimeError, match="22 keypoint rows past the packet"):
        g.gather_async(*t, keyps=kt[:10]).finish()
    # nothing past the packet: finish adds no section
    roomy = ResultGatherer(F, D, 28, 1, "cpu", with_masks=False, keyps_k=K, keyps_rows=32)
    assert "keyps_extra" not in roomy.gather_async(*t, keyps=kt).finish()


# --------------------------------------------------------------------------- #
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANK_COUNTS = ([3, 0, 9], [7, 16, 10])  # 12 and 33 rows


def _worker(rank, world, port, outq):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vosdetectron_amd.runner import ResultGatherer, frame_keyps
    dets, cls, counts, keyps = _rank_outputs(rank, counts=RANK_COUNTS[rank])
    t = _t((dets, cls, counts))
    kt = torch.from_numpy(keyps)
    g = ResultGatherer(3, 16, 28, world, "cpu", with_masks=False, keyps_k=K, keyps_rows=40)
    out = g.gather(*t, keyps=kt)
    got = {k: v.numpy().copy() for k, v in out.items()}
    got["per_frame"] = [frame_keyps(out, 3, i).numpy().copy() for i in range(world * 3)]
    # rank 1 alone overflows (33 rows vs 30): rank 0 sends zero padding
    one = ResultGatherer(3, 16, 28, world, "cpu", with_masks=False, keyps_k=K, keyps_rows=30)
    fin = one.gather_async(*t, keyps=kt).finish()
    got["extra_shape"] = tuple(fin["keyps_extra"].shape)
    got["extra_rank0_zero"] = not bool(fin["keyps_extra"][0].any())
    got["over_frames"] = [frame_keyps(fin, 3, i).numpy().copy() for i in range(world * 3)]
    outq.put((rank, got))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_keyps_world2_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    exp = [_rank_outputs(r, counts=RANK_COUNTS[r]) for r in range(world)]
    for rank in range(world):  # every rank holds the same, rank-major result
        got = res[rank]
        assert np.array_equal(got["dets"], np.concatenate([e[0] for e in exp]))
        assert np.array_equal(got["classes"], np.concatenate([e[1] for e in exp]))
        assert np.array_equal(got["counts"], np.concatenate([e[2] for e in exp]))
        assert got["keyps"].shape == (world, 40, 4, K)
        assert got["extra_shape"] == (world, 3, 4, K) and got["extra_rank0_zero"]
        for r, (d, c, n, kp) in enumerate(exp):
            assert np.array_equal(got["keyps"][r, :len(kp)], kp)
            o = 0
            for f in range(3):
                assert got["keyps_offsets"][r, f] == o
                assert np.array_equal(got["per_frame"][r * 3 + f], kp[o:o + n[f]])
                assert np.array_equal(got["over_frames"][r * 3 + f], kp[o:o + n[f]])
                o += n[f]
