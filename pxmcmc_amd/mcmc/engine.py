"""The stepping engine of the samplers and estimators: static buffers, an iteration counter, HIP-graph replay between
observable events.  A host's ``_engine_start`` builds an :class:`Engine`, sets ``one`` and whichever hooks it needs, and
calls ``ready``."""
import torch

from .. import ops


def capture(warm, restore, bodies):
    """Capture one HIP graph per callable of ``bodies`` -- the only place the samplers capture.  ``warm()`` runs first,
    outside capture on a side stream (lazy allocations, attributes); ``restore()`` then puts the state back and each
    body is captured under ``ops.capture_scope()``: a plan torn down while a capture is in progress (the garbage
    collector may run at any point) only queues its device frees, which the library empties at the end of the scope.
    Capture does not execute, so the state is the restored one afterwards.  Returns (graphs, None), or, when capture
    fails, (None, repr(exc)) with the state restored: eager stepping, same results."""
    try:
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            warm()
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        restore()
        graphs = []
        for body in bodies:
            g = torch.cuda.CUDAGraph()
            with ops.capture_scope(), torch.cuda.graph(g):
                body()
            graphs.append(g)
        return graphs, None
    except Exception as exc:  # capture unsupported in this environment
        restore()
        return None, repr(exc)


class _Counter:
    """iteration counter of the engines that step on the operators' own plans (the fused engines use the plan's
    ops.IterCounter): a device int64 ``t`` that the noise kernels read when they run (graph replay), or, with
    ``host=True``, a host int ``i`` that the eager-only engine passes to each call"""

    def __init__(self, start, host=False):
        self.i = int(start)
        self.t = None if host else torch.full((1,), self.i, dtype=torch.int64, device=ops.device())

    def set(self, v):
        self.i = int(v)
        if self.t is not None:
            self.t.fill_(self.i)

    def add(self, inc=1):
        if self.t is None:
            self.i += inc
        else:
            ops.counter_add(self.t, inc)

    def close(self):
        pass


class Engine:
    """
    Every attribute the engine ever holds; the builder sets ``one`` and whichever hooks it needs.

    * ``XA``, ``XB``   -- ping-pong state buffers: the state is in XA (side "A") or XB (side "B");
    * ``side``         -- which of XA / XB holds the current state; replays start from XA (``advance`` realigns first);
    * ``P``            -- forward(state): written by every step, or formed on demand (``form_preds``);
    * ``form_preds``   -- ``form_preds(X)`` writes P of the state X; set when the steps do not write P;
    * ``P_stale``      -- P lags the state (set by ``advance``, cleared by ``state``; with ``form_preds`` only);
    * ``one``          -- ``one(src, dst)``: one iteration from the state in src to dst;
    * ``cnt``          -- iteration counter read by the steps: the plan's ops.IterCounter, or a :class:`_Counter`;
    * ``cnt0``         -- ``cnt0(i)``: counter value at which the next step is iteration i (the ring step shifts it);
    * ``reset``        -- rebuilds plan-carried state from (XA, P) after a restore;
    * ``plan``         -- WavPlan of the fused steps (None: the steps run on the operators' own plans);
    * ``pairs``        -- state and preds carried pair-packed (MYULA real_pairs); ``unpack`` then maps them to [C, .];
    * ``ring``         -- fused ring-space step (scalar sig_d);
    * ``graph``        -- captured graph of 2 iterations (None: eager stepping);
    * ``graph_long``   -- captured graph of 2 * GRAPH_PAIRS iterations;
    * ``graph_error``  -- repr of the exception that made capture fall back to eager stepping.

    ``eng[name]`` is ``eng.name``, for the benchmark and the tests; the library uses the attributes.
    """

    GRAPH_PAIRS = 4  # iterations per graph replay = 2 * GRAPH_PAIRS (fewer, longer launches of the host)

    def __init__(self, X, preds, cnt, plan=None, pairs=False, unpack=None):
        self.XA, self.XB, self.side = X.clone(), torch.empty_like(X), "A"
        self.P, self.form_preds, self.P_stale = preds.clone(), None, False
        self.one, self.cnt, self.cnt0, self.reset = None, cnt, (lambda i: i), (lambda: None)
        self.plan, self.pairs, self.unpack, self.ring = plan, pairs, unpack, False
        self.graph = self.graph_long = self.graph_error = None

    def __getitem__(self, key):
        return getattr(self, key)

    def __setitem__(self, key, value):
        setattr(self, key, value)

    def ready(self, X, preds, i0, graph_ok):
        """point the counter at iteration i0 and, if ``graph_ok``, capture the graphs of 2 and 2 * GRAPH_PAIRS
        iterations; (X, preds) is the start state as the engine carries it"""
        self.cnt.set(self.cnt0(i0))
        if graph_ok:
            XA, XB, one = self.XA, self.XB, self.one

            def two():
                one(XA, XB)
                one(XB, XA)

            def restore():
                XA.copy_(X)
                self.P.copy_(preds)
                self.cnt.set(self.cnt0(i0))
                self.reset()

            bodies = [lambda n=n: [two() for _ in range(n)] for n in (1, self.GRAPH_PAIRS)]
            graphs, self.graph_error = capture(two, restore, bodies)
            self.graph, self.graph_long = graphs or (None, None)
        return self

    def advance(self, k):
        """advance the state by k iterations (graph replays of 2 * GRAPH_PAIRS + eager remainder)"""
        if k > 0 and self.form_preds is not None:
            self.P_stale = True
        if self.side == "B" and k > 0:  # realign so that replays start from XA
            self.one(self.XB, self.XA)
            self.side = "A"
            k -= 1
        if self.graph is not None:
            per = 2 * self.GRAPH_PAIRS
            while k >= per:
                self.graph_long.replay()
                k -= per
            while k >= 2:
                self.graph.replay()
                k -= 2
        while k >= 2:
            self.one(self.XA, self.XB)
            self.one(self.XB, self.XA)
            k -= 2
        if k == 1:
            self.one(self.XA, self.XB)
            self.side = "B"

    def state(self):
        """(X, preds) of the current state as [C, .] arrays (pair-packed engines unpack here: observation only)"""
        X = self.XA if self.side == "A" else self.XB
        if self.P_stale:  # preds on demand: forward(X) of the current state
            self.form_preds(X)
            self.P_stale = False
        # observation point: the host is about to read the state -- an expired device wait since the last one raises
        if self.plan is not None:
            self.plan.raise_on_fault()
        if self.pairs:
            return self.unpack(X), self.unpack(self.P)
        return X, self.P

    def stop(self):
        """unregister the iteration counter and drop the buffers, graph and closures (the closures reference the
        host: without this the plan would only be released by a later garbage collection)"""
        if self.cnt is not None:
            self.cnt.close()
            self.graph = self.graph is not None  # keep the flags (ring, pairs, graph) for inspection
            for k in ("one", "XA", "XB", "P", "form_preds", "unpack", "plan", "cnt", "cnt0", "graph_long", "reset"):
                setattr(self, k, None)
