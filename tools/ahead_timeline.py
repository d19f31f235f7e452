"""Where do forward k's decoder and forward k + 1's encoder run in time?  The bench workload's pipelined pair step (two
buckets, reuse events), a few steps back to back behind a run that keeps the host ahead, timed by the executor's OWN events
(the diagnostic-mark mechanism of tools/branch_times.py): per forward the head's end ([7], side stream), the ahead chain's
begin and end ([14], [13], ahead stream), the main chain's begin behind the join ([15]) and the forward's end (an event of
ours on the main stream), and the overlap of forward k's main chain with forward k + 1's ahead chain.
With one chain (IMF_ENCODER_AHEAD=0, or a library without an ahead stream) the ahead marks stay unrecorded: the tool then
prints the head's end and the forwards' ends only.   usage: python tools/ahead_timeline.py [passes of two forwards, default 15]"""
import os, sys
os.environ["IMFNET_DIAG_EVENTS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch
import bench
from imfnet_amd import _lib
L = _lib.lib()
PASSES = int(sys.argv[1]) if len(sys.argv) > 1 else 15
dev = torch.device("cuda:0")
model, sd = bench.build_model(dev)
pts, imgs = bench.load_pair(1.7)
if os.environ.get("SINGLE"):
    pts, imgs = pts[:1], imgs[:1]
wl = bench.Workload(model, dev, pts, imgs, 0.025)
us = lambda a, b: L.imf_event_elapsed_ms(a, b) * 1e3        # -1000 when an event was never recorded
with torch.no_grad():
    wl.prepare_graph(pipelined=True)
    wl.runner.use_graph = False
    for _ in range(60): wl.graph_step()
    torch.cuda.synchronize()
    # what the steps DID, not what the rule says: without an ahead stream (ops.ahead_stream found none) they keep one chain
    went_ahead = all(getattr(b, "last_ahead", False) for b in wl.buckets)
    ahead = L.imf_resunet_encoder_ahead(int(wl.runner.variant), len(pts)) if went_ahead else 0
    from imfnet_amd import ops
    print("; ".join(ops.AHEAD_NOTES.values()) or "no ahead stream was asked for")
    rows = []
    for rep in range(PASSES):
        for _ in range(6): wl.graph_step()                  # the host runs ahead of the device, as in the bench's steps
        ends, t0 = [], L.imf_event_create()
        L.imf_event_record(t0, wl.stream.cuda_stream)
        # (a bucket's marks are overwritten by its next forward: two forwards per pass, one per bucket, read pass by pass)
        for k in range(2):
            wl.graph_step()
            e = L.imf_event_create(); L.imf_event_record(e, wl.stream.cuda_stream); ends.append(e)
        torch.cuda.synchronize()
        ev = [wl.buckets[(wl._turn - 2 + k) % 2].events for k in range(2)]
        rec = []
        for k in range(2):
            if ahead > 0:
                rec += [us(t0, ev[k][7]), us(t0, ev[k][14]), us(t0, ev[k][13]), us(t0, ev[k][15]), us(t0, ends[k])]
            else:
                rec += [us(t0, ev[k][7]), float("nan"), float("nan"), float("nan"), us(t0, ends[k])]
        rows.append(rec)
        for e in ends + [t0]: L.imf_event_destroy(e)
r = np.median(np.array(rows), axis=0)
print("ahead launches per forward: %d (0 = one chain); medians over %d passes, us since the first forward's issue point on the main stream" % (ahead, len(rows)))
for k in range(2):
    h, a0, a1, m0, m1 = r[5 * k:5 * k + 5]
    print("forward %d: head done %7.1f | ahead chain %7.1f -> %7.1f (%6.1f) | main chain %7.1f -> %7.1f (%6.1f)"
          % (k, h, a0, a1, a1 - a0, m0, m1, m1 - m0))
if ahead > 0:
    # forward 0's main chain against forward 1's ahead chain
    lo, hi = max(r[3], r[6]), min(r[4], r[7])
    print("forward 1's ahead chain runs %.1f us of its %.1f us under forward 0's main chain (%.1f us); forward 1 ends %.1f us after forward 0 (two forwards into a drained queue: not the steady step)"
          % (max(0.0, hi - lo), r[7] - r[6], r[4] - r[3], r[9] - r[4]))
