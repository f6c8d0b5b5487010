"""Per-shape frame plan: the steady-state frame (stereo -> motion -> fusion) captured once into a
hipGraph and replayed per frame.

The reference runs ~3 500-4 000 eager launches per frame; here a frame is
~600 launches of hand-written kernels whose host-side issue cost (ctypes + Python) would still
dominate at 30 fps, so the whole frame is recorded with HIP stream capture
(torch.cuda.CUDAGraph drives hipStreamBeginCapture/EndCapture and owns the capture-time memory
pool).  Recurrent state (reference model/codd.py:322-366: memory, raft_feat, raft_netinp) lives
in static buffers that the graph reads at its head and overwrites at its tail.
"""
import torch

from . import ops


class FrameRunner:
    """Runs ConsistentOnlineDynamicDepth frame by frame on one GPU, eagerly or by graph replay."""

    def __init__(self, estimator, img_metas, use_graph=True, check_finite=False):
        self.est = estimator
        self.metas = img_metas
        self.use_graph = use_graph
        # debug aid: a host-synchronising isfinite check of every frame's output -- the fp16 operand formats
        # (--precision fp16 | split16 | fp16mix) saturate to +-inf above 65504 and nothing else guards against it at run time
        self.check_finite = check_finite
        self.last = {}  # per-frame side outputs of the last step (e.g. "Ts", the SE3 field: scene-flow evaluation)
        self.state = {}
        self.graph = None
        self._static = None
        self.frames = 0

    def reset(self):
        """New sequence (reference reset_inference_state, model/codd.py:400-433)."""
        self.state = {}
        self.frames = 0
        if self._static is not None:
            self._static["primed"] = False

    # ---- eager ------------------------------------------------------------------------------
    def _eager(self, left, right):
        out = self.est.consistent_online_depth_estimation(left, right, self.metas, self.state)
        self.last = {k: out[k] for k in ("Ts",) if out.get(k) is not None}
        return out["pred_disp"]

    # ---- graph ------------------------------------------------------------------------------
    def _state_tensors(self, state):
        mem = state["memory"]
        return [mem[0], mem[1], mem[2], state["raft_feat"], state["raft_netinp"]]

    def _capture(self, left, right):
        dev = left.device
        st = dict(l=torch.empty_like(left), r=torch.empty_like(right), primed=True)
        st["state"] = [torch.empty_like(t).contiguous() for t in self._state_tensors(self.state)]
        for dst, src in zip(st["state"], self._state_tensors(self.state)):
            dst.copy_(src)
        st["l"].copy_(left)
        st["r"].copy_(right)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()

        def body():
            s = st["state"]
            state = dict(memory=[s[0], s[1], s[2]], raft_feat=s[3], raft_netinp=s[4])
            out = self.est.consistent_online_depth_estimation(st["l"], st["r"], self.metas, state)
            # state write-back with a KERNEL, not Tensor.copy_: under capture copy_/memset become
            # memcpy/memset graph nodes, and on ROCm 7.2 a captured hipMemsetAsync node was observed
            # to race with the neighbouring kernel nodes (GPU page faults after ~45 replays when
            # eager work ran between replays).  Only kernel nodes are used inside the frame graph.
            ops.copy_many([(dst, src.contiguous()) for dst, src in zip(s, self._state_tensors(state))])
            st["last"] = {k: out[k] for k in ("Ts",) if out.get(k) is not None}  # (lives in the graph's memory pool)
            return out["pred_disp"]

        saved = [t.clone() for t in st["state"]]
        with torch.cuda.stream(stream):
            body()  # warm-up on the side stream (weight packing, allocator)
            for dst, src in zip(st["state"], saved):
                dst.copy_(src)
            torch.cuda.synchronize(dev)
            with torch.cuda.graph(g, stream=stream):
                st["out"] = body()
        torch.cuda.current_stream(dev).wait_stream(stream)
        # capture does not execute: restore the pre-capture state and replay once for this frame
        for dst, src in zip(st["state"], saved):
            dst.copy_(src)
        self.graph, self._static = g, st

    def eager_frame_on_static_state(self, left, right):
        """One eager (un-captured) steady-state frame on the current recurrent state -- used by
        bench.py to bracket individual launches with events.  Advances the state."""
        if self.est.motion is None and self.est.fusion is None:  # stereo-only estimator: no recurrent state
            return self._eager(left, right)
        if self._static is not None and self._static.get("primed"):
            s = self._static["state"]
            state = dict(memory=[s[0], s[1], s[2]], raft_feat=s[3], raft_netinp=s[4])
        else:
            state = self.state
        out = self.est.consistent_online_depth_estimation(left, right, self.metas, state)
        if state is not self.state:
            for dst, src in zip(self._static["state"], self._state_tensors(state)):
                dst.copy_(src)
        return out["pred_disp"]

    def _capture_stateless(self, left, right):
        """Stereo-only estimator (no motion / fusion, BASELINE.json configs[1]): no recurrent state."""
        dev = left.device
        st = dict(l=left.clone(), r=right.clone(), primed=True, state=[])
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            self._eager(st["l"], st["r"])  # warm-up (weight packing, allocator)
            torch.cuda.synchronize(dev)
            with torch.cuda.graph(g, stream=stream):
                st["out"] = self._eager(st["l"], st["r"])
        torch.cuda.current_stream(dev).wait_stream(stream)
        self.graph, self._static = g, st

    def step_fill(self, fill, scratch):
        """One frame whose inputs the caller writes in place: ``fill(left, right)`` must enqueue, on the current
        stream, the writes of this frame's normalised images into the two [B,3,H,W] buffers it is given.  Once the
        frame graph is live those are the graph's own static inputs, so the frame costs no device-to-device copy
        (codd_amd.live feeds camera frames this way); until then (the eager first frame, the capturing second one,
        the re-priming frame after reset()) they are ``scratch = (left, right)``, the caller's own buffers, and the
        frame goes through ``step`` unchanged.  Same result and same validity as ``step``."""
        st = self._static
        stateless = self.est.motion is None and self.est.fusion is None
        if not self.use_graph or self.graph is None or not (stateless or st["primed"]):
            fill(*scratch)
            return self.step(*scratch)
        self.frames += 1
        fill(st["l"], st["r"])
        self.graph.replay()
        if stateless:
            return st["out"]
        self.state = {"memory": True}
        self.last = st.get("last", {})
        if self.check_finite and not bool(torch.isfinite(st["out"]).all()):
            raise FloatingPointError(f"frame {self.frames}: non-finite disparity (conv precision {ops.CONV_PRECISION})")
        return st["out"]

    def step(self, left, right):
        """One frame.  Returns the (fused) disparity [B,1,H,W]; valid until the next call."""
        self.frames += 1
        if self.use_graph and self.est.motion is None and self.est.fusion is None:
            if self.graph is None:
                self._capture_stateless(left, right)
            self._static["l"].copy_(left, non_blocking=True)
            self._static["r"].copy_(right, non_blocking=True)
            self.graph.replay()
            return self._static["out"]
        has_mem = "memory" in self.state or (self._static is not None and self._static.get("primed"))
        if not self.use_graph or not has_mem:
            d = self._eager(left, right)
            return d
        if self.graph is None:
            self._capture(left, right)
        elif not self._static["primed"]:
            for dst, src in zip(self._static["state"], self._state_tensors(self.state)):
                dst.copy_(src)
            self._static["primed"] = True
        st = self._static
        st["l"].copy_(left, non_blocking=True)
        st["r"].copy_(right, non_blocking=True)
        self.graph.replay()
        self.state = {"memory": True}  # state now lives in the static buffers
        self.last = st.get("last", {})
        if self.check_finite and not bool(torch.isfinite(st["out"]).all()):
            raise FloatingPointError(f"frame {self.frames}: non-finite disparity (conv precision {ops.CONV_PRECISION})")
        return st["out"]
