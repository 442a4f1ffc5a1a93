"""HIP-graph capture for the decode samplers (``compile_on_decode`` / ``graphed``): the one place in
owl_wms that captures a graph.

``capture`` records a callable on a side stream.  ``StepGraph`` is the pattern the samplers share: ONE
Euler step on static buffers, replayed for every step -- the cache is read-only while a frame is
denoised, so every step launches the same kernels on the same buffers; same kernels and arithmetic as
the eager loop (the reference's ``compile_on_decode`` switch).  ``FrameGraph`` is the
ring streams' other pattern: a whole streamed frame, the cache's commit included, as one graph.

What a caller has to keep to (the graph knows nothing about samplers, models or RoPE):

* step 0 of the first frame runs eagerly BEFORE the capture: it creates the per-weight bf16 copies and
  the workspaces outside the graph's memory pool;
* a replayed step reads its cache position from the device, so the caller checks it on the host
  (nn.attn.check_rope_rows) before each replayed frame, as the eager step's attention does;
* ``dt`` is a static device scalar, rewritten per step (``StepGraph.replay``).
"""
import torch


def capture(fn, pool=None):
    """Record fn() on a side stream into a new graph (in memory pool `pool`, else a private one); the
    side stream waits for the work queued so far and the current stream for the capture.
    -> (graph, fn's result)."""
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, pool=pool, stream=side):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return g, out


def _release_graph(g):
    """Destroy a step graph only after its queued replays have run: its exec (kernel arguments) and
    its private memory pool are released here, so no replay of it may still be queued then."""
    torch.cuda.current_stream().synchronize()
    g.reset()


class StepGraph:
    """One step ``step(state, inputs, dt) -> new state`` captured on static buffers.  `state` and `inputs`
    are dicts of named tensors, cloned here into the static buffers; the step gets the buffers under the
    same names and returns the new state's tensors in `state`'s order, which the capture writes back into
    the state buffers.  `dt` is cloned into the static scalar."""

    def __init__(self, step, state, inputs, dt, pool=None):
        self._state = tuple(state)
        self.bufs = {k: v.clone() for k, v in {**state, **inputs}.items()}
        self.dt = dt.clone()

        def body():
            new = step({k: self.bufs[k] for k in self._state}, {k: self.bufs[k] for k in inputs}, self.dt)
            for k, v in zip(self._state, new):
                self.bufs[k].copy_(v)

        self.graph, _ = capture(body, pool)

    def load(self, **tensors):
        """fresh values for the named buffers (a new frame's state and inputs)"""
        for k, v in tensors.items():
            self.bufs[k].copy_(v)

    def replay(self, dt):
        self.dt.copy_(dt)
        self.graph.replay()

    def state(self):
        """clones of the state buffers, in `state`'s order"""
        return tuple(self.bufs[k].clone() for k in self._state)

    def release(self):
        _release_graph(self.graph)


class FrameGraph:
    """One whole streamed frame ``frame(inputs) -> outputs`` captured on static buffers (the ring streams'
    ``graphed="frame"``): `inputs` is a dict of named tensors, cloned here into the static buffers the
    frame function gets under the same names; its outputs (a tuple of tensors) stay in the graph's pool
    and are cloned out per replay.  Everything that changes between frames is either an input or device
    state the frame's own kernels read and advance (the ring position), so a frame is copy-in, one
    replay, clone-out.  The capture executes nothing."""

    def __init__(self, frame, inputs, pool=None):
        self.bufs = {k: v.clone() for k, v in inputs.items()}
        self.graph, self.out = capture(lambda: tuple(frame(self.bufs)), pool)

    def load(self, **tensors):
        """fresh values for the named buffers (a new frame's noise and controls)"""
        for k, v in tensors.items():
            self.bufs[k].copy_(v)

    def replay(self):
        self.graph.replay()

    def outputs(self):
        """clones of the frame function's outputs, in its order"""
        return tuple(o.clone() for o in self.out)

    def release(self):
        _release_graph(self.graph)
