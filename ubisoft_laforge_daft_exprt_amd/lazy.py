"""A dict of a few numbers that live in one device tensor and are fetched with ONE host transfer on first access."""
from __future__ import annotations


class DeviceDict(dict):
    """Subclasses name their ``KEYS``; ``_values(host tensor)`` turns the fetched tensor into one value per key (default: its elements as
    Python numbers).  Until something reads a value nothing is transferred, so a loop that only logs every n-th step never stalls the
    stream.  Comparison with ``==`` fetches first."""

    KEYS = ()

    def __init__(self, device_terms):
        super().__init__()
        self._device_terms = device_terms

    def _values(self, host):
        return host.tolist()

    def _fetch(self):
        if self._device_terms is not None:
            host = self._device_terms.cpu()
            self._device_terms = None
            super().update(zip(self.KEYS, self._values(host)))

    def __getitem__(self, k):
        self._fetch()
        return super().__getitem__(k)

    def __iter__(self):
        self._fetch()
        return super().__iter__()

    def __len__(self):
        return len(self.KEYS)

    def __contains__(self, k):
        return k in self.KEYS

    def __eq__(self, other):
        self._fetch()
        if isinstance(other, DeviceDict):
            other._fetch()
        return super().__eq__(other)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def keys(self):
        self._fetch()
        return super().keys()

    def items(self):
        self._fetch()
        return super().items()

    def values(self):
        self._fetch()
        return super().values()

    def get(self, k, default=None):
        self._fetch()
        return super().get(k, default)

    def __repr__(self):
        self._fetch()
        return super().__repr__()
