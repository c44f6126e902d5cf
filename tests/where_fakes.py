"""numpy TEST DOUBLE of the attribute columns and ``where`` for the CPU tests of the sharded index:
``facets_fakes.FakeFacetIndex`` plus the attribute slots.  ``where`` is ``flat_index.where_numpy`` over the stored
columns and ``facets(by_attribute=)`` the double's own ``facets`` over the stored column, so the sharded code is
compared with one index holding all rows.  It lives in tests/ only; the product never falls back to it."""
import numpy as np

from claude_semantic_search_amd.flat_index import ATTR_F32, ATTR_I32, attr_slot, attr_values, where_args, where_numpy
from facets_fakes import FakeFacetIndex


class FakeWhereIndex(FakeFacetIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._attrs = {}

    def _default(self, typ, n):
        return np.full(n, np.nan, np.float32) if typ == ATTR_F32 else np.full(n, -1, np.int32)

    def add(self, x, normalize=False):
        super().add(x, normalize)
        for slot, col in self._attrs.items():     # rows added later start at the default
            typ = ATTR_F32 if col.dtype == np.float32 else ATTR_I32
            self._attrs[slot] = np.concatenate([col, self._default(typ, self.ntotal - col.shape[0])])

    def set_attribute(self, slot, values, row0=0):
        slot = attr_slot(slot)
        a, typ = attr_values(values)
        assert 0 <= row0 and row0 + a.shape[0] <= self.ntotal
        self.calls.append(("set_attribute", slot, int(row0), int(a.shape[0])))
        if a.shape[0] == 0:
            return
        col = self._attrs.setdefault(slot, self._default(typ, self.ntotal))
        if col.dtype != a.dtype:
            raise RuntimeError(f"attribute slot {slot} holds {col.dtype} values")
        col[row0:row0 + a.shape[0]] = a

    def get_attribute(self, slot, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        col = self._attrs.get(slot)
        return (self._default(ATTR_I32, self.ntotal) if col is None else col)[row0:row0 + n].copy()

    def attribute_type(self, slot):
        col = self._attrs.get(attr_slot(slot, "attribute_type"))
        return -1 if col is None else (ATTR_F32 if col.dtype == np.float32 else ATTR_I32)

    def drop_attribute(self, slot):
        self._attrs.pop(slot, None)

    def where(self, clauses, allow=None, return_count=False):
        where_args(clauses, self.attribute_type)
        self.calls.append(("where", len(list(clauses)), allow is not None))
        mask = where_numpy(self._attrs, clauses, self.ntotal, allow=allow)
        return (mask, int(mask.sum())) if return_count else mask

    def facets(self, q, thresh, buckets=None, nbuckets=None, normalize=False, allow=None, by_attribute=None):
        if by_attribute is None:
            return super().facets(q, thresh, buckets=buckets, nbuckets=nbuckets, normalize=normalize, allow=allow)
        assert buckets is None and nbuckets is not None and self.attribute_type(by_attribute) == ATTR_I32
        return super().facets(q, thresh, buckets=self._attrs[by_attribute], nbuckets=nbuckets, normalize=normalize, allow=allow)
