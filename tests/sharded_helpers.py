"""What the emulated-rank tests of the sharded step share: a rank's slice of a
particle store, and the ranks' exported stores put back together in rank order.
The ranks themselves run under phdslam.dist.LocalWorld, the in-process
transport; the order of a step's phases is ShardedFilter's."""
import numpy as np


def _cat_offsets(parts):
    o = [0]
    for p in parts:
        o.extend((np.asarray(p[1:]) + o[-1]).tolist())
    return np.asarray(o, dtype=np.int32)


def slice_store(state, lo, hi):
    """Particles lo .. hi-1 of a static store (poses, lw, maps, offs)."""
    poses, lw, maps, offs = state
    o = offs[lo:hi + 1]
    return poses[lo:hi].copy(), lw[lo:hi].copy(), maps[o[0]:o[-1]].copy(), (o - o[0]).astype(np.int32)


def gathered_store(filters):
    """The ranks' static stores in rank order as one (poses, lw, maps, offs)."""
    got = [f.export() for f in filters]
    return (np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]),
            np.concatenate([g[2] for g in got]), _cat_offsets([g[3] for g in got]))


def slice_mixed(poses, lw, sm, sof, dm, dof, lo, hi):
    """Particles lo .. hi-1 of a mixed store (static and dynamic maps)."""
    so, do = sof[lo:hi + 1], dof[lo:hi + 1]
    return (poses[lo:hi].copy(), lw[lo:hi].copy(), sm[so[0]:so[-1]].copy(), (so - so[0]).astype(np.int32),
            dm[do[0]:do[-1]].copy(), (do - do[0]).astype(np.int32))


def gathered_mixed(filters):
    """The ranks' stores in rank order as one (poses, lw, sm, sof, dm, dof)."""
    dyn = [f.export_dynamic() for f in filters]
    return (*gathered_store(filters), np.concatenate([d[0] for d in dyn]), _cat_offsets([d[1] for d in dyn]))
