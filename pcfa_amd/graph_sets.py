"""What one attacked image pair leaves to the next pair of the same key, and the per-model caches that keep it.

attack_l2 and attack_FGSM.attack loop over a batch-1 loader (attack_PCFA.py:668-670) and every KITTI / Sintel pair has the
same size: the static device buffers a captured closure reads and writes, the hipGraphs themselves and (for L-BFGS) the
optimiser whose flat gradient buffer the closure fills survive the pair.  The next pair of the same key adopts them, copies
its images / initial variables / target in and pays no warm-up and no re-capture.

A model carries one plain dict per attack (`cache`), key -> GraphSet, least recently used first.  A set has ONE live owner:
`adopt` retires the previous one, `put` the owners of the sets it evicts.  Config.max_cached_shapes counts the sets of ONE
lane (attack_PCFA.PairsInFlight): a lane's new shape evicts an older shape of the same lane, never another lane's live set.
Each set pins a closure graph pool and, for L-BFGS, a 2 x 101 x n history (~1.1 GB at 440x1024)."""
import logging
import weakref

# the attribute on the model that holds each attack's dict (tests and tools clear these by name)
CACHES = {"pair-graph": "_pcfa_pair_graphs", "pair-batch-graph": "_pcfa_pair_batch_graphs",
          "fgsm-graph": "_pcfa_fgsm_graphs"}


class GraphSet:
    """The attributes `names` of `owner` -- static buffers, graphs, optimiser -- under their own names, the one live attack
    that uses them (`owner`, a weak reference), its lane, and how many pairs have used / captured the set."""

    def __init__(self, owner, lane, names):
        self.names = tuple(names)
        for name in self.names:
            setattr(self, name, getattr(owner, name))
        self.owner = weakref.ref(owner)
        self.lane = lane
        self.pairs = 1
        self.captures = 1          # stays 1 however many pairs adopt the set

    def retire_owner(self):
        st = self.owner()
        if st is not None:
            st._retire()

    def drop(self):
        """Evicted: let go of the graphs (and their memory pools) and of the optimiser's history."""
        self.graphed = self.repredict = self.optimizer = None


def cache(model, what):
    """The dict of `what` (a key of CACHES) on `model`; a model that takes no attribute gets a throw-away one."""
    kept = getattr(model, CACHES[what], None)
    if kept is None:
        kept = {}
        try:
            object.__setattr__(model, CACHES[what], kept)   # plain attribute: not a module / parameter
        except Exception:  # noqa: BLE001
            return {}
    return kept


def _log_eviction(what, key):
    logging.warning("pcfa_amd: %s cache full: dropping the graph set of %r -- the next pair of that shape pays warm-up + "
                    "capture again (raise Config.max_cached_shapes / PCFA_MAX_CACHED_SHAPES if this repeats)", what, key)


def put(sets, key, kept, cap, what):
    """Insert `kept` as the most recently used set (dicts keep insertion order) and evict the oldest sets of ITS lane beyond
    `cap`: their owners are retired first -- they must not replay graphs whose buffers are about to go."""
    sets.pop(key, None)
    sets[key] = kept
    mine = [k for k, s in sets.items() if s.lane == kept.lane]
    for old_key in mine[:max(0, len(mine) - max(1, int(cap)))]:
        old = sets.pop(old_key)
        _log_eviction(what, old_key)
        old.retire_owner()
        old.drop()


def adopt(sets, key, owner):
    """The set kept under `key` (None if there is none) handed to `owner`: the previous owner, if still alive, is retired
    -- the buffers, graphs and optimiser state are the new pair's now -- and the set becomes the most recently used."""
    kept = sets.pop(key, None)
    if kept is None:
        return None
    sets[key] = kept
    kept.retire_owner()
    kept.owner = weakref.ref(owner)
    kept.pairs += 1
    for name in kept.names:
        setattr(owner, name, getattr(kept, name))
    return kept
