"""Writes tests/golden/discriminators_launches.json: every library call the HiFi-GAN discriminators make, argument for argument, for the
module forwards, ``losses``, ``generator_loss_grad`` and ``discriminator_loss_grad`` at B = 2 and T = 12 and 257, first and repeated
calls.  tests/test_discriminators_launches_cpu.py records again and requires equality: equal calls into an unchanged library are the same
bits, so a change to the host side that is meant to change nothing is checked on the CPU.

Runs on the CPU with no library loaded.  ``_lib.lib()`` hands out a recorder (so ``discriminators.lib()`` and every helper it calls do),
torch's current stream is a constant, and the "there is no CPU path" guard of discriminators.py is switched off by name (``GUARDS``).
Which arguments are pointers is read from include/daft_exprt_hip.h (``_lib.parse_header``), never from a table kept here.  No address
reaches the file: the parameters and buffers are named by state-dict key ('msd.discriminators.1.convs.2.bias+0'), the waveforms 'y' and
'y_hat', the tensors handed to ``refresh_weights`` 'folded:<key>.w' / '.b', every other tensor 'buf<k>:<its size in bytes>+<byte offset>', k in
the order of first use; the recorder keeps every tensor it has named, so no address is used twice.  A size query's output is 'out', and the query answers
16 (1 + the sum of its scalar arguments mod 97), so that the code's ``max`` over its workspace requests shows in the later calls.  The
first ``dx_disc_losses`` call on a table carries the table's rows, pointers named, as one more element.

To keep the file reviewable, the calls are written out, one per line, at T = 257 in f32 (every period pads) for the four entries in
which something is built (``FULL``); of every other entry and case the file holds the call count and the SHA-256 of the same lines
(``digest``).  Equal digests are equal calls; ``python tests/golden/make_golden_discriminators_launches.py --full FILE`` writes every case out in full,
to be diffed against the same dump of another commit.

The file was written ONCE, from discriminators.py as it stood before its layer table (the four separate layer walks), and is not
regenerated from later code.  That commit had four guards instead of one; it was recorded with this script and

    GUARDS = ('_check_run', '_check_differentiable', '_check_train')
    disc._LossPlan.__init__ = <a copy of it without its device test>

    python tests/golden/make_golden_discriminators_launches.py
"""
import bisect
import ctypes
import hashlib
import json
import os
import sys
import weakref

import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(os.path.dirname(HERE)) not in sys.path:         # run as a script: the package is two directories up
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import disc_helpers as dh  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import _lib, discriminators as disc  # noqa: E402

OUT = os.path.join(HERE, 'discriminators_launches.json')
CASES = [(T, precision) for T in (12, 257) for precision in ('f32', 'bf16')]
# what the file writes out call by call: at T = 257 in f32, the four entries in which something is built
FULL = {'T257-f32': ('losses', 'generator_loss_grad', 'discriminator_loss_grad', 'losses_after_refresh_folded')}
GUARDS = ('_require_gpu',)
STREAM_HANDLE = 77


def _span(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + max(s.nbytes(), 1)


class LiveTensors(TorchDispatchMode):
    """Notes, weakly, every tensor an operator returns while the mode is on: how an address finds the tensor it points into."""

    def __init__(self):
        super().__init__()
        self.refs = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.refs += [weakref.ref(t) for t in (out if isinstance(out, (tuple, list)) else (out,)) if torch.is_tensor(t)]
        return out

    def find(self, p):
        self.refs = [r for r in self.refs if r() is not None]
        for r in reversed(self.refs):
            t = r()
            if t is not None and _span(t)[0] <= p < _span(t)[1]:
                return t
        raise AssertionError(f'a pointer argument ({p:#x}) lies in no live tensor')


class Names:
    """address -> 'name+offset'; a tensor not named yet becomes the next 'buf<k>', and is kept alive from then on."""

    def __init__(self, live):
        self.live, self.los, self.spans, self.k = live, [], [], 0

    def add(self, name, t):
        lo, hi = _span(t)
        i = bisect.bisect_right(self.los, lo)
        self.los.insert(i, lo)
        self.spans.insert(i, (hi, name, t))

    def __call__(self, p):
        i = bisect.bisect_right(self.los, p) - 1
        if i < 0 or p >= self.spans[i][0]:
            t = self.live.find(p)
            self.add(f'buf{self.k}:{t.untyped_storage().nbytes()}', t)
            self.k += 1
            i = bisect.bisect_right(self.los, p) - 1
        return f'{self.spans[i][1]}+{p - self.los[i]}'


class Recorder:
    """Stands in for the library: an entry point of the header is a function that notes [name, arguments...] and returns 0."""

    def __init__(self, names):
        self.calls, self.names, self.tables = [], names, set()
        self.protos = _lib.parse_header(with_names=True)

    def __getattr__(self, entry):
        _, argtypes, argnames = self.protos[entry]
        query = entry.endswith(('_size', '_workspace'))

        def call(*args):
            assert len(args) == len(argtypes), entry
            answer = 16 * (1 + sum(a for a, t in zip(args, argtypes) if t is not ctypes.c_void_p) % 97)
            out = [entry]
            for a, t, n in zip(args, argtypes, argnames):
                if n == 'stream':
                    assert a == STREAM_HANDLE, entry
                    out.append('stream')
                elif t is not ctypes.c_void_p or a is None:
                    out.append(a)
                elif query:
                    ctypes.c_long.from_address(a).value = answer
                    out.append('out')
                else:
                    out.append(self.names(a))
            if entry == 'dx_disc_losses' and out[1] not in self.tables:
                self.tables.add(out[1])
                rows = (ctypes.c_int64 * (4 * args[1])).from_address(args[0])
                out.append([[self.names(rows[4 * i]), self.names(rows[4 * i + 1]), rows[4 * i + 2], rows[4 * i + 3]] for i in range(args[1])])
            self.calls.append(out)
            return 0
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


class _Stream:
    cuda_stream = STREAM_HANDLE


def record(T, precision):
    """-> {entry: [[entry point, arguments...], ...]} for one input length and precision, in the order the entries are made."""
    noop = lambda *args, **kwargs: None
    saved = [(_lib, '_LIB', _lib._LIB), (torch.cuda, 'current_stream', torch.cuda.current_stream)] + [(disc, g, getattr(disc, g)) for g in GUARDS]
    live = LiveTensors()
    names = Names(live)
    rec = Recorder(names)
    out = {}
    try:
        _lib._LIB, torch.cuda.current_stream = rec, (lambda device=None: _Stream)
        for g in GUARDS:
            setattr(disc, g, noop)
        with live:
            y, y_hat = dh.make_inputs(T, 1)
            D = disc.HiFiGanDiscriminators(dh.state_dicts(), device='cpu', precision=precision)
            names.add('y', y)
            names.add('y_hat', y_hat)
            for tag, module in (('mpd', D.mpd), ('msd', D.msd)):
                for key, t in module.state_dict().items():
                    names.add(f'{tag}.{key}', t)
            with torch.no_grad():
                D.mpd(y, y_hat)
                out['forward_mpd'] = rec.take()
                D.msd(y, y_hat)
                out['forward_msd'] = rec.take()
            D.mpd.refresh_weights()                    # the forwards built the packs: the first losses() below builds them again
            D.msd.refresh_weights()
            with torch.no_grad():
                for again in ('', '_again'):
                    D.losses(y, y_hat)
                    out['losses' + again] = rec.take()
            for again in ('', '_again'):
                D.generator_loss_grad(y, y_hat)
                out['generator_loss_grad' + again] = rec.take()
            if precision == 'f32':
                D.discriminator_loss_grad(y, y_hat, power_iterations=1)
                out['discriminator_loss_grad'] = rec.take()
                D.discriminator_loss_grad(y, y_hat, power_iterations=0, folded=True)
                out['discriminator_loss_grad_folded'] = rec.take()
                for tag, module in (('mpd', D.mpd), ('msd', D.msd)):
                    F = {}
                    for key, m in module.named_modules():
                        if hasattr(m, 'weight_g'):
                            F[key] = (torch.zeros_like(m.weight_v), torch.zeros_like(m.bias))
                            names.add(f'folded:{tag}.{key}.w', F[key][0])
                            names.add(f'folded:{tag}.{key}.b', F[key][1])
                    module.refresh_weights(F)
                with torch.no_grad():
                    D.losses(y, y_hat)
                out['losses_after_refresh_folded'] = rec.take()
    finally:
        for owner, name, value in saved:
            setattr(owner, name, value)
    return out


def record_all():
    return {f'T{T}-{precision}': record(T, precision) for T, precision in CASES}


def _line(call):
    return json.dumps(call, separators=(',', ':'))


def digest(calls):
    """-> {'calls': n, 'sha256': of the lines ``dumps`` would write for them}"""
    return {'calls': len(calls), 'sha256': hashlib.sha256('\n'.join(_line(call) for call in calls).encode()).hexdigest()}


def dumps(recorded, full=FULL):
    """One line per call for the entries in ``full`` (None: all), so that a mismatch reads as a diff; one line per entry, its digest, for
    the others."""
    lines = ['{']
    for i, (key, rec) in enumerate(recorded.items()):
        lines.append(f' {json.dumps(key)}: {{')
        for j, (entry, calls) in enumerate(rec.items()):
            if full is None or entry in full.get(key, ()):
                lines.append(f'  {json.dumps(entry)}: [')
                lines += ['   ' + _line(call) + (',' if k + 1 < len(calls) else '') for k, call in enumerate(calls)]
                lines.append('  ]' + (',' if j + 1 < len(rec) else ''))
            else:
                lines.append(f'  {json.dumps(entry)}: {json.dumps(digest(calls))}' + (',' if j + 1 < len(rec) else ''))
        lines.append(' }' + (',' if i + 1 < len(recorded) else ''))
    lines.append('}')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    recorded = record_all()
    whole = '--full' in sys.argv
    with open(sys.argv[sys.argv.index('--full') + 1] if whole else OUT, 'w') as f:
        f.write(dumps(recorded, None if whole else FULL))
    for key, rec in recorded.items():
        print(key + ': ' + ', '.join(f'{entry} {len(calls)}' for entry, calls in rec.items()))
