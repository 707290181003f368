"""The one recipe for a captured HIP graph ("One graph cache"): static input buffers, a warm-up outside the capture, the
capture itself, a keyed cache with a size limit and a victim rule; the site then copies its inputs in and replays."""
import torch


def warm_up(fn):
    """``fn()`` on a fresh side stream, fenced against the current stream before and after: kernel attributes, weight packs and the
    allocator settle outside the capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return out


def capture(fn, pool=None):
    """``fn()`` captured -> (graph, what fn returned).  ``pool``: another graph's ``pool()``, to share its memory."""
    graph = torch.cuda.CUDAGraph()
    # thread_local: CUDA calls of OTHER threads (the RCCL watchdog polling its events, a pinned-memory loader) must not abort the capture
    with torch.cuda.graph(graph, pool=pool, capture_error_mode='thread_local'):
        out = fn()
    return graph, out


class Entry:
    """What one key caches: ``graphs`` (a list, replayed in order), ``hits`` (counted by the site, per graphed call) and the site's own
    static inputs and captured outputs as attributes."""

    def __init__(self, graphs, **fields):
        self.graphs, self.hits = graphs, 0
        self.__dict__.update(fields)


class GraphCache(dict):
    """key -> Entry, at most ``limit`` of them: inserting a new key into a full cache first drops one victim (its pool is freed with it),
    the entry with the fewest ``hits`` ('least_used'; the first inserted among equals) or the first inserted ('oldest')."""

    def __init__(self, limit, evict):
        if evict not in ('least_used', 'oldest'):
            raise ValueError(f"evict must be 'least_used' or 'oldest', got {evict!r}")
        super().__init__()
        self.limit, self.evict = limit, evict

    def __setitem__(self, key, entry):
        if key not in self and len(self) >= self.limit:
            del self[next(iter(self)) if self.evict == 'oldest' else min(self, key=lambda k: self[k].hits)]
        super().__setitem__(key, entry)
