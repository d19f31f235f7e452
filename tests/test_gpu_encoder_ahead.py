"""Ahead mode (imf_fragment_io.ahead_stream): forward k + 1's encoder on a fourth stream beside forward k's decoder.

Workloads: the fixture pair at scale 1.0 and 5 cm (a few thousand voxels per fragment, one or two tiles on the stride-8 level)
as ONE forward, and one fragment per forward (another kernel policy, the level-0 twin only); weights from seeded_state_dict.
Two DIFFERENT inputs of one capacity key alternate over two buckets -- the pair and the pair in swapped order (or fragment 0
and fragment 1) -- so a stale buffer or an early overwrite changes a result.  Every comparison is torch.equal / == against the
same input's one-bucket forward.

`python tests/test_gpu_encoder_ahead.py N_ITEMS` is the child of the IMF_ENCODER_AHEAD=0 comparison: it prints the digests of
the same ten forwards as one JSON line."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

VOXEL, SCALE, STEPS = 0.05, 1.0, 10


class Rig:
    """Three buckets of one capacity key on the runner's streams: [0] holds input A, [1] input B, [2] takes the references."""

    def __init__(self, n_items):
        import bench
        self.dev = dev = torch.device("cuda:0")
        self.n_items = n_items
        self.model, _ = bench.build_model(dev)
        pts, imgs = bench.load_pair(SCALE)
        if n_items == 2:
            raw = [([pts[0], pts[1]], imgs[[0, 1]]), ([pts[1], pts[0]], imgs[[1, 0]])]
        else:
            raw = [([pts[0]], imgs[:1]), ([pts[1]], imgs[1:2])]
        self.runner = r = self.model.fragment_runner()
        assert r is not None
        r.use_graph = False
        self.inputs = []
        with torch.no_grad():
            for plist, im in raw:                      # one exact forward per input teaches the runner its capacities
                wl = bench.Workload(self.model, dev, plist, im.copy(), VOXEL)
                wl.exact_step()
                torch.cuda.synchronize()
                cm = wl.last_st.coordinate_manager
                lv = [cm.level(ts) for ts in (1, 2, 4, 8)]
                r.observe(int(wl.xyz.shape[0]), [l.n for l in lv], lv[0].bbox)
                if n_items > 1:
                    r.observe_batch(n_items, lv[0].bbox)
                self.inputs.append((wl.xyz, wl.starts, wl.img))
        n_max = max(int(x.shape[0]) for x, _, _ in self.inputs)
        H, W = int(imgs.shape[2]), int(imgs.shape[3])
        key = r.caps_for(n_max, n_items, H, W, VOXEL, True)
        assert key is not None
        self.stream = r.main_stream(dev)
        self.buckets = [r.bucket(key, dev, self.stream, lane="ahead-test-%d" % i) for i in range(3)]
        for b, inp in zip(self.buckets[:2], self.inputs):
            self.stage(b, inp)
        torch.cuda.synchronize()
        # A stream to go ahead on, unconditionally: the runner's (ops.ahead_stream keeps one only if it runs beside the other
        # three), else one of our own -- the bits do not depend on which hardware queue the stream landed on, only the speed does.
        self.own_stream = None
        ahead = r.ahead_stream(dev)
        if not ahead:
            ahead = self.own_stream = r.L.imf_stream_create()
        assert ahead
        for b in self.buckets:
            b.ahead_stream = ahead
        self.ahead_rule = int(r.L.imf_resunet_encoder_ahead(int(r.variant), n_items))   # (0 in the IMF_ENCODER_AHEAD=0 child)
        self.refs = [self.one_bucket(inp) for inp in self.inputs]   # computed once, never written again

    def stage(self, b, inp):
        xyz, starts, img = inp
        return self.runner.stage(b, xyz, starts, img, self.stream)

    def one_bucket(self, inp, trace=None):
        """The input's forward alone in bucket [2], head and encoder on the main stream: (descriptors, counts, flags)."""
        b = self.buckets[2]
        n = self.stage(b, inp)
        with torch.no_grad():
            res = self.runner.launch(b, n, self.n_items, self.stream, trace_list=trace)
        torch.cuda.synchronize()
        return res.F.clone(), res.counts, res.flags

    def issue(self, steps):
        """`steps` back-to-back forwards alternating buckets [0] / [1] with reuse events (bench.py's pipelined pattern); the
        outputs are cloned on the main stream right behind each call; nothing here synchronises."""
        done, out = [None, None], []
        with torch.no_grad():
            for k in range(steps):
                b = self.buckets[k % 2]
                reuse = done[k % 2]
                if reuse is None:
                    reuse = torch.cuda.Event()
                    reuse.record(self.stream)
                res = self.runner.launch(b, int(self.inputs[k % 2][0].shape[0]), self.n_items, self.stream, reuse_event=reuse)
                with torch.cuda.stream(self.stream):
                    clone = b.out.clone()
                e = torch.cuda.Event()
                e.record(self.stream)                  # behind the clone: the last reader of this bucket's outputs
                done[k % 2] = e
                out.append((res, clone, b.last_ahead))
        return out

    @staticmethod
    def collect(out):
        torch.cuda.synchronize()
        return [(clone[: res.counts[0]], res.counts, res.flags, ahead) for res, clone, ahead in out]

    def pipelined(self, steps):
        """issue + ONE synchronise: [(descriptors, counts, flags, went ahead)] per forward."""
        return self.collect(self.issue(steps))


_RIGS = {}


def rig(n_items):
    if n_items not in _RIGS:
        _RIGS[n_items] = Rig(n_items)
    return _RIGS[n_items]


def digest(F, counts, flags):
    h = hashlib.sha256(F.cpu().numpy().tobytes())
    h.update(np.asarray(list(counts) + [flags], np.int64).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("n_items", [2, 1])
def test_alternating_inputs_over_two_buckets_equal_their_one_bucket_forwards(n_items):
    """Ten back-to-back forwards, two inputs, two buckets, the encoder of each on the ahead stream: descriptors, counts and flags
    of every one equal its input's one-bucket forward; a fresh process with IMF_ENCODER_AHEAD=0 (one chain) gets the same bits."""
    g = rig(n_items)
    assert g.ahead_rule > 0                                                     # bf16x3, one or two fragments: ahead by default
    assert g.refs[0][1][0] > 1000 * n_items                                     # a few thousand voxels per fragment
    assert not torch.equal(g.refs[0][0][:256], g.refs[1][0][:256])              # the two inputs do differ
    stats0 = g.runner.stats["ahead"]
    outs = g.pipelined(STEPS)
    for k, (F, counts, flags, ahead) in enumerate(outs):
        Fr, cr, fr = g.refs[k % 2]
        assert flags == fr == 0 and counts == cr, (k, counts, cr, flags)
        assert torch.equal(F, Fr), "forward %d differs from its one-bucket reference" % k
        assert ahead is True, "forward %d kept one chain" % k
    assert g.runner.stats["ahead"] - stats0 == STEPS
    mine = [digest(F, c, f) for F, c, f, _ in outs]
    env = dict(os.environ, IMF_ENCODER_AHEAD="0")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), str(n_items)], env=env, capture_output=True, text=True,
                           timeout=180)
    assert child.returncode == 0, child.stderr[-2000:]
    theirs = json.loads(child.stdout.strip().splitlines()[-1])
    assert theirs["ahead"] == 0 and theirs["digests"] == mine


@pytest.mark.parametrize("n_items", [2, 1])
def test_work_on_the_callers_stream_behind_the_call_sees_finished_descriptors(n_items):
    """The main stream carries the end of an ahead forward: a clone enqueued on it right behind the call, with nothing but one
    final synchronise, holds the reference (Rig.pipelined clones exactly so; here the LAST forward of a short run is the point)."""
    g = rig(n_items)
    F, counts, flags, ahead = g.pipelined(3)[-1]
    Fr, cr, fr = g.refs[0]
    assert g.ahead_rule > 0 and ahead is True
    assert counts == cr and flags == fr and torch.equal(F, Fr)


@pytest.mark.parametrize("n_items", [2, 1])
def test_launches_without_a_reuse_event_and_traced_steps_keep_one_chain(n_items):
    """A launch without a reuse event carries head_on_side == 0 and no ahead stream and issues nothing ahead; a traced step
    right behind pipelined ones (no synchronise in between) equals the reference."""
    g = rig(n_items)
    g.pipelined(4)
    b = g.buckets[0]
    before = g.runner.stats["ahead"], g.runner.L.imf_fragment_ahead_forwards()
    with torch.no_grad():
        issued = g.issue(3)                                                      # work of both buckets still queued ...
        res = g.runner.launch(b, int(g.inputs[0][0].shape[0]), n_items, g.stream)
        with torch.cuda.stream(g.stream):
            clone = b.out.clone()
    outs = g.collect(issued)
    n_ahead = 3
    assert g.ahead_rule > 0 and all(ahead is True for _, _, _, ahead in outs)
    assert b.io.head_on_side == 0 and not b.io.ahead_stream and not b.io.reuse_event and b.last_ahead is False
    assert (g.runner.stats["ahead"], g.runner.L.imf_fragment_ahead_forwards()) == (before[0] + n_ahead, before[1] + n_ahead)
    assert res.flags == 0 and res.counts == g.refs[0][1] and torch.equal(clone[: res.counts[0]], g.refs[0][0])
    assert all(torch.equal(F, g.refs[k % 2][0]) for k, (F, _, _, _) in enumerate(outs))
    # ... and a traced step (its own bucket, every convolution between two events) behind a fresh run of pipelined ones
    issued = g.issue(2)
    tr = []
    F, counts, flags = g.one_bucket(g.inputs[1], trace=tr)
    assert all(torch.equal(Fk, g.refs[k % 2][0]) for k, (Fk, _, _, _) in enumerate(g.collect(issued)))
    assert len(tr) > 15 and flags == 0 and counts == g.refs[1][1] and torch.equal(F, g.refs[1][0])
    assert g.buckets[2].last_ahead is False


if __name__ == "__main__":
    g = Rig(int(sys.argv[1]))
    outs = g.pipelined(STEPS)
    print(json.dumps(dict(ahead=g.runner.stats["ahead"], digests=[digest(F, c, f) for F, c, f, _ in outs])))
