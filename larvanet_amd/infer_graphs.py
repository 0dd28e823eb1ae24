"""Which grad-free forward a call runs (Form) and the rule that decides when its shape is worth a hipGraph (GraphTable).
Neither touches the GPU: the plugin (inference.InferenceMixin._eager_or_graph) hands the table the callables that do."""
from typing import NamedTuple


class _FormPair(NamedTuple):
    u8: bool = False
    ensemble: bool = False


class Form(_FormPair):
    """uint8 [N][H][W][3] in and out (u8) or float [N][3][H][W]; the x8 self-ensemble or the plain forward; every exit's
    image ([M] in front of the batch: exits) or the route's end alone.  Decided once at the entry point and passed down as
    one value.  As a tuple it stays the pair (u8, ensemble) that callers unpack; `exits` rides along as an attribute and
    takes part in equality."""

    def __new__(cls, u8=False, ensemble=False, exits=False):
        self = super().__new__(cls, u8, ensemble)
        self.exits = bool(exits)
        return self

    def __eq__(self, other):
        return tuple(self) == tuple(other) and self.exits == getattr(other, "exits", False)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple(self), self.exits))

    def __repr__(self):
        return "Form(u8=%r, ensemble=%r, exits=%r)" % (self.u8, self.ensemble, self.exits)


class GraphTable(dict):
    """key -> what capture(x) returned for it: a callable that replays the captured forward on a new x, or False for a
    capture that failed (never retried).  A key seen once runs eagerly -- validation images all differ in size --; seen
    for the second time it is captured, unless the table already holds `limit` entries."""

    def __init__(self, limit=4):
        super().__init__()
        self.limit = limit
        self.seen = {}

    def clear(self):
        super().clear()
        self.seen.clear()

    def forward(self, key, x, capture, run):
        ent = self.get(key)
        if ent is None:
            if len(self.seen) > 512:   # (a long run over images of ever new sizes: forget the counts)
                self.seen.clear()
            self.seen[key] = self.seen.get(key, 0) + 1
            if self.seen[key] < 2 or len(self) >= self.limit:
                return run(x)
            ent = self[key] = capture(x)
        return run(x) if ent is False else ent(x)
