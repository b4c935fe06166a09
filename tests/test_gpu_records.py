"""What the migration-record kernels move (csrc/phd_records.hip), compared
byte for byte, on the two paths no other test reads back: the slots form of
the receive (phd_shard_receive) and the pack whose record count lives on the
device (phd_shard_resample with a send buffer).  Static PHD, CPHD and the mixed
static + dynamic store share one set of kernels; every comparison is byte
equality, no tolerance is involved.

n = 8 particles, map capacity 16 (one mixed case 15), dynamic capacity 8 (rows
of whole 16-byte quads: the vector copy) or 6 (the scalar copy).  Particle 1
has an empty static and an empty dynamic map, particle 5 full ones; the others
lie between (particles 6 / 7: one map empty, the other full).
"""
import numpy as np
import pytest

from phdslam.scenario import mixed_config, mixed_scenario

N_PART = 8
SSZ = [8, 0, 3, 15, 5, 16, 0, 16]  # static components per particle at capacity 16
DSZ = [4, 0, 1, 7, 3, 8, 8, 0]     # dynamic components at dynamic capacity 8
# (model, map capacity, dynamic capacity).  The context accepts an odd map
# capacity: with 15 the static part is 113 words, so three padding words
# precede the dynamic part.
CASES = [("phd", 16, 0), ("cphd", 16, 0), ("mixed", 16, 8), ("mixed", 16, 6), ("mixed", 15, 8)]


def _truncate(maps, stride, sizes):
    """Particle p keeps the first sizes[p] of its `stride` components."""
    keep = np.concatenate([np.arange(p * stride, p * stride + s) for p, s in enumerate(sizes)]).astype(np.int64)
    return maps[keep], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _input(model, cap, dcap):
    """(cfg, store, z): store = [poses, lw, static maps, offsets(, dynamic maps, offsets)]."""
    import phdslam
    n = N_PART
    lw = np.random.default_rng(3).normal(-8, 3, n).astype(np.float32)
    ssz = [min(s, cap) for s in SSZ]
    if model == "mixed":
        cfg = mixed_config(resampleThresh=1.0)
        poses, sm, _, dm, _, z = mixed_scenario(cfg, n, cap, dcap, 6, seed=4242)
        dsz = [dcap if s == 8 else min(s, dcap) for s in DSZ]
        assert 0 in dsz and dcap in dsz
        store = [poses, lw, *_truncate(sm, cap, ssz), *_truncate(dm, dcap, dsz)]
    else:
        cfg, poses, _, maps, offs, z = phdslam.config_scenario(2 if model == "phd" else 3, n=n, G=cap, M=4)
        cfg.resampleThresh = 1.0
        np.testing.assert_array_equal(np.diff(offs), cap)
        store = [poses, lw, *_truncate(maps, cap, ssz)]
    assert 0 in ssz and cap in ssz
    return cfg, store, z


def _reversed(store):
    """The same particles in reverse order: other poses, weights and maps in every slot."""
    out = [store[0][::-1].copy(), store[1][::-1].copy()]
    for k in range(2, len(store), 2):
        m, o = store[k], store[k + 1]
        out.append(np.concatenate([m[o[p]:o[p + 1]] for p in range(len(o) - 2, -1, -1)]))
        out.append(np.concatenate([[0], np.cumsum(np.diff(o)[::-1])]).astype(np.int32))
    return out


def _context(model, cfg, cap, dcap, store, z):
    import phdslam
    f = phdslam.PHDFilter(N_PART, cfg, map_capacity=cap, max_measurements=8, candidate_capacity=512,
                          survivor_capacity=64)
    f.set_seed(1234)
    f.set_check_each_update(False)  # (a full map overflows on an update: truncated the same way on both sides)
    if model == "mixed":
        f.enable_dynamic(dcap)
    f.load(*store[:4])
    if model == "mixed":
        f.load_dynamic(*store[4:])
    if model == "cphd":  # a CPHD update leaves cardinality coefficients to carry (test_particle_records_round_trip)
        f.set_step_births(0)
        _update(f, model, z)
    return f


def _update(f, model, z):
    if model == "cphd":
        f.set_measurements(z)
        f.predict_update(None, 0, do_predict=False)
    else:
        f.update(z)


FIELDS = ("pose", "log-weight", "static map", "cardinality row", "dynamic map")


def _particles(f, model):
    """Per particle (pose, log-weight, static map, cardinality row, dynamic map) as bytes."""
    poses, lw, maps, offs = f.export()
    n = len(poses)
    cn = f.cardinality_distribution() if model == "cphd" else np.zeros((n, 0), np.float32)
    dm, do = f.export_dynamic() if model == "mixed" else (np.zeros(0, np.uint8), np.zeros(n + 1, np.int32))
    return [(poses[p].tobytes(), lw[p].tobytes(), maps[offs[p]:offs[p + 1]].tobytes(), cn[p].tobytes(),
             dm[do[p]:do[p + 1]].tobytes()) for p in range(n)]


def _assert_particle(got, want, label):
    for g, w, name in zip(got, want, FIELDS):
        assert g == w, f"{label}: {name} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("model,cap,dcap", CASES)
def test_receive_slots_content(gpu, model, cap, dcap):
    """phd_shard_receive: context A packs its 8 particles, context B (loaded
    with the particles in reverse order) takes records [1, 1, 4, 5, 5, 5] into
    slots 2..7.  Those slots then hold A's particles 1, 1, 4, 5, 5, 5 — pose,
    log-weight, static map, the CPHD cardinality row, the dynamic map — and
    slots 0..1 what B was loaded with; after one update with the same scan on
    both they still do, so the slabs of the sets X that slots share are read
    correctly.  Records 1 and 5 are the empty and the full maps (CPHD: the
    sizes its first update left, of which one is empty and one full)."""
    import torch
    n = N_PART
    slot_rec, first = [1, 1, 4, 5, 5, 5], 2
    cfg, store, z = _input(model, cap, dcap)
    a = _context(model, cfg, cap, dcap, store, z)
    b = _context(model, cfg, cap, dcap, _reversed(store), z)
    dev = torch.device("cuda", 0)
    rb = a.record_bytes()
    assert rb == b.record_bytes()
    rec = torch.zeros(n * rb, dtype=torch.uint8, device=dev)
    a.pack(torch.arange(n, dtype=torch.int32, device=dev).data_ptr(), n, rec.data_ptr())
    torch.cuda.synchronize()  # (the two contexts run on their own streams)
    pa, pb0 = _particles(a, model), _particles(b, model)
    sizes = [len(pa[r][2]) // 28 for r in slot_rec]  # (a Gaussian2D is 7 floats)
    print(f"{model} cap {cap} dcap {dcap}: static sizes of the records {sizes}, record {rb} bytes")
    assert 0 in sizes and cap in sizes
    if model == "mixed":
        dsizes = [len(pa[r][4]) // 84 for r in slot_rec]
        assert 0 in dsizes and dcap in dsizes
        dyn_at = (4 * (8 + 7 * cap) + 15) // 16 * 16
        assert rb == (dyn_at + 16 + 84 * dcap + 15) // 16 * 16
        assert dyn_at - 4 * (8 + 7 * cap) == (12 if cap == 15 else 0)  # padding before the dynamic part
    b.shard_receive(rec.data_ptr(), torch.tensor(slot_rec, dtype=torch.int32, device=dev).data_ptr(), len(slot_rec),
                    first)
    for when in ("after the receive", "after one update"):
        pa, pb = _particles(a, model), _particles(b, model)
        for i, r in enumerate(slot_rec):
            _assert_particle(pb[first + i], pa[r], f"{when}: slot {first + i} (record {r})")
        if when == "after the receive":
            for s in range(first):
                _assert_particle(pb[s], pb0[s], f"{when}: slot {s} (not received)")
            _update(a, model, z)
            _update(b, model, z)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model,cap,dcap", [("phd", 16, 0), ("mixed", 16, 8)])
def test_device_count_pack_content(gpu, model, cap, dcap):
    """phd_shard_resample with a send buffer (the record count is read on the
    device, the records carry the new log-weight): rank 0 of an emulated world
    of 2 x 8 particles holds 90 % of the weight, so it sends its surplus.  The
    first sum(send_records) records of the zeroed buffer equal what
    phd_pack_particles writes for the same index list on a twin context that
    was not resampled, but for word 6 (the log-weight), which is the new
    log-weight; the records beyond stay zero."""
    import torch
    n, world = N_PART, 2
    N = n * world
    cfg, store, z = _input(model, cap, dcap)
    f = _context(model, cfg, cap, dcap, store, z)
    twin = _context(model, cfg, cap, dcap, store, z)
    f.set_measurements(z)
    dev = torch.device("cuda", 0)
    rb = f.record_bytes()
    assert rb == twin.record_bytes() and rb % 4 == 0
    w = torch.from_numpy(np.concatenate([np.full(n, np.log(0.9 / n)), np.full(n, np.log(0.1 / n))]).astype(np.float32)).to(dev)
    new_lw = np.float32(-np.log(N))
    parents = torch.empty(N, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    send = torch.zeros(n * (world - 1), dtype=torch.int32, device=dev)
    recv = torch.empty(n, dtype=torch.int32, device=dev)
    records = torch.zeros(n * rb, dtype=torch.uint8, device=dev)
    _, rs, _, snd, _ = f.shard_resample(w.data_ptr(), world, 0, 0x5eed, 3, parents.data_ptr(), keep.data_ptr(),
                                        send.data_ptr(), recv.data_ptr(), records.data_ptr(), n, float(new_lw))
    torch.cuda.synchronize()
    cnt = sum(snd)
    src = send.cpu().numpy()[:cnt]
    print(f"{model}: {cnt} records sent, particles {src.tolist()}")
    assert rs and 2 <= cnt < n  # (a condition on the input: other weights if it fails)
    want = torch.zeros(cnt * rb, dtype=torch.uint8, device=dev)
    twin.pack(send.data_ptr(), cnt, want.data_ptr())
    twin.synchronize()
    got = records.cpu().numpy().view(np.uint32).reshape(n, rb // 4)
    want = want.cpu().numpy().view(np.uint32).reshape(cnt, rb // 4)
    assert not got[cnt:].any(), "records beyond the device's count were written"
    assert got[:cnt, 6].tobytes() == np.full(cnt, new_lw, np.float32).tobytes()
    assert want[:, 6].tobytes() == store[1][src].tobytes()  # (the twin's records carry its own log-weights)
    got[:cnt, 6] = want[:, 6]
    assert got[:cnt].tobytes() == want.tobytes()
    f.close()
    twin.close()
