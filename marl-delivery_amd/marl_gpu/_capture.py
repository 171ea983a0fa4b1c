"""The one hipGraph capture/replay path of the device-resident collectors ("The graph rule").

A collector's ``collect(graph=True)`` runs eagerly once, captures the same work with ``capture``,
and keeps the graph in a ``GraphCache``.  A graph reads its modules' parameters, its buffers and an
action tape in place, so the cache hands it back only for the very same owner objects (strong
references, compared by identity) whose parameters still live at the captured addresses
(``load_state_dict`` copies in place; rebinding ``param.data`` does not) and for equal plain values
(step counts, flags).

The offset rule: the sampler's offset base lives on the device (``_off_dev``, uint64 bits in an
int64 tensor [1]).  A captured region draws at ``_off_dev[0] + k`` and ends with
``mdl_counter_add(_off_dev, steps)``, so a graph replayed several times in one call keeps counting.
``Graphed._replay`` writes the host ``offset`` into ``_off_dev`` before the call's first replay and
advances ``offset`` afterwards: the host int stays the one truth, and eager calls, graphed calls
and plain assignments to ``offset`` interleave freely.
"""
from __future__ import annotations

import contextlib

import torch


def capture(device, fn):
    """Capture ``fn()`` on a side stream as one hipGraph.  Returns (graph, fn's return value).
    Capture runs nothing: the caller restores whatever host counters ``fn`` advanced."""
    torch.cuda.synchronize(device)
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = fn()
    torch.cuda.current_stream(device).wait_stream(s)
    torch.cuda.synchronize(device)
    return g, out


def param_addresses(*objs):
    """The addresses a graph over ``objs`` reads in place: ``data_ptr()`` of every parameter of an
    object with ``parameters()``, a tensor's own; a string or a plain callable has none."""
    out = []
    for o in objs:
        if isinstance(o, torch.Tensor):
            out.append(o.data_ptr())
        elif hasattr(o, "parameters"):
            out.extend(q.data_ptr() for q in o.parameters())
    return tuple(out)


class GraphCache:
    """The graphs captured for one key (owner objects, their parameter addresses, plain values), by
    slot.  A string owner (the evaluator's "greedy") is matched by value: it has no object."""

    def __init__(self):
        self.clear()

    def clear(self):
        self._owners, self._addresses, self._values = (), (), None
        self._graphs = {}            # slot -> (graph, steps)

    def matches(self, owners, values) -> bool:
        """True if graphs are kept and were captured for exactly this key."""
        return (bool(self._graphs) and len(owners) == len(self._owners)
                and all(a is b or (isinstance(a, str) and a == b) for a, b in zip(owners, self._owners))
                and param_addresses(*owners) == self._addresses and tuple(values) == self._values)

    def lookup(self, owners, values, slot=None):
        """The graph stored for this key and slot, or None."""
        return self._graphs[slot][0] if self.matches(owners, values) and slot in self._graphs else None

    def store(self, owners, values, slot, graph, steps: int):
        """Keep ``graph`` (``steps`` steps long).  A new key drops the graphs of the old one."""
        if not self.matches(owners, values):
            self._owners, self._addresses, self._values = tuple(owners), param_addresses(*owners), tuple(values)
            self._graphs = {}
        self._graphs[slot] = (graph, int(steps))

    def __len__(self):
        return len(self._graphs)

    def captured_graphs(self) -> dict:
        """{slot: steps} of the graphs kept."""
        return {slot: steps for slot, (_, steps) in self._graphs.items()}


class Graphed:
    """What a collector with graphs holds: the host ``offset``, its device copy and the cache."""

    def _init_graphs(self, device):
        self.offset = 0
        self._off_dev = torch.zeros(1, dtype=torch.int64, device=device)   # offset base (uint64 bits)
        self._graphs = GraphCache()

    def captured_graphs(self) -> dict:
        """{slot: steps} of the hipGraphs kept for ``graph=True`` (slot None where there is one graph)."""
        return self._graphs.captured_graphs()

    def _replay(self, graphs, steps: int):
        """The offset rule around one call's replays: ``graphs`` run in order from ``offset``, which
        then advances by ``steps`` (the draws the graphs consumed)."""
        self._off_dev.fill_(self.offset)
        for g in graphs:
            g.replay()
        self.offset += steps


@contextlib.contextmanager
def eval_mode(*modules):
    """Run the block with every object that has ``eval`` / ``train`` in eval mode; afterwards (also
    after an exception) those that were training train again.  Other objects pass through."""
    were_training = [m for m in modules if hasattr(m, "eval") and hasattr(m, "train") and getattr(m, "training", False)]
    for m in modules:
        if hasattr(m, "eval") and hasattr(m, "train"):
            m.eval()
    try:
        yield
    finally:
        for m in were_training:
            m.train()
