"""BGZF files inflated on the GPU (``vrx_bgzf_*``, csrc/vrx_bgzf.h).

cellSNP and ``bgzip`` write a .vcf.gz as a chain of independent gzip members of at most 64 KiB of text; each names
its compressed size in its header and the CRC32 and length of its text in its footer.  One wavefront inflates one
member and holds it to that footer.  The contract: the caller gets the bytes ``gzip.open(path).read()`` gives, or a
``BgzfStatus`` that names what the device could not vouch for, and then reads the file with Python's ``gzip``, which
raises what it always raised for a corrupt file.  ``last()`` tells which way the most recent file went.

``load_donor_GPb`` and ``read_cellVCF`` inflate BGZF files here by default (profiles/bgzf_bench.json: faster than
``gzip`` at every shape measured); ``VIREO_INFLATE=host`` makes them use ``gzip``, ``VIREO_INFLATE=device`` names the
default.  Plain gzip files have one deflate stream and stay on the host.
"""
import ctypes as C
import os
import time

import numpy as np

from . import _lib

DEFAULT = "device"                # what the readers do without VIREO_INFLATE (README; profiles/bgzf_bench.json)
BATCH_BYTES = 256 << 20           # text of one vrx_bgzf_inflate call: the readers' slab
_HEADER = b"\x1f\x8b\x08\x04"
_SCAN_STATUS = {1: "a member that does not begin with bgzip's 18 header bytes", 2: "a member cut short",
                3: "a member size BGZF does not allow"}
_MEMBER_STATUS = ((1, "the stream runs past the payload"), (2, "block type 3"), (4, "a stored block's NLEN"),
                  (8, "a code-length header"), (16, "an over-subscribed code"), (32, "an incomplete code"),
                  (64, "no end-of-block code"), (128, "an invalid symbol"), (256, "a distance before the first byte"),
                  (512, "text beyond ISIZE"), (1024, "less text than ISIZE"), (2048, "payload bytes left over"),
                  (4096, "CRC32"), (8192, "the iteration cap"), (16384, "ISIZE"))

_last = None


class BgzfStatus(Exception):
    """The device does not vouch for this file; ``reason`` says why.  The caller inflates it on the host."""

    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


def last():
    """The record of the most recent file: dict(file, path 'device' | 'host', reason (None on the device path),
    members, seconds dict(scan, upload, kernels, download)); None before the first."""
    return None if _last is None else dict(_last, seconds=dict(_last['seconds']))


def _record(name, path, reason=None, members=0):
    global _last
    _last = dict(file=name, path=path, reason=reason, members=members,
                 seconds=dict(scan=0.0, upload=0.0, kernels=0.0, download=0.0))
    return _last


def note_host(name, reason):
    """A reader inflates ``name`` with gzip: the decision is never silent."""
    _record(name, 'host', reason)


def is_bgzf(path):
    """Does the file begin with a BGZF member header (1f 8b 08 04, XLEN 6, subfield BC of length 2)?"""
    with open(path, "rb") as fh:
        h = fh.read(18)
    return len(h) == 18 and h[:4] == _HEADER and h[10:16] == b"\x06\x00BC\x02\x00"


def wanted():
    """what VIREO_INFLATE asks of the readers: 'device' or 'host'"""
    mode = os.environ.get("VIREO_INFLATE", DEFAULT)
    if mode not in ("device", "host"):
        raise ValueError("VIREO_INFLATE is 'device' or 'host', not %r" % mode)
    return mode


def scan(image):
    """The members of a BGZF file image (bytes-like) -> dict(status 0 | 1 | 2 | 3, members, payload_off, payload_len,
    isize, out_off (members + 1: where each member's text begins, then the total)); host code only."""
    L = _lib.lib()
    buf = np.frombuffer(image, dtype=np.uint8)
    ptr = buf.ctypes.data_as(_lib._U8) if len(buf) else None
    n, st = C.c_int64(0), C.c_int32(0)
    _lib.check(L.vrx_bgzf_scan(ptr, len(buf), 0, C.byref(n), None, None, None, None, C.byref(st)))
    m = n.value
    off, length = np.zeros(m, np.int64), np.zeros(m, np.int32)
    isize, out_off = np.zeros(m, np.int32), np.zeros(m + 1, np.int64)
    if m:
        _lib.check(L.vrx_bgzf_scan(ptr, len(buf), m, C.byref(n), off.ctypes.data_as(_lib._I64),
                                   length.ctypes.data_as(_lib._I32), isize.ctypes.data_as(_lib._I32),
                                   out_off.ctypes.data_as(_lib._I64), C.byref(st)))
    return dict(status=st.value, members=m, payload_off=off, payload_len=length, isize=isize, out_off=out_off)


def _member_reason(status):
    return ", ".join(text for bit, text in _MEMBER_STATUS if status & bit)


class BgzfReader:
    """The text of a BGZF file, inflated on the device a batch of members at a time: ``read(n)`` and ``close()`` as
    of a file object.  ``batch_bytes``: text per batch (64 KiB ... 1 GiB, default 256 MiB).  Raises ``BgzfStatus``,
    from the constructor for a file that is not a clean chain of BGZF members, from ``read`` for a member that
    fails one of the decoder's checks.  ``statuses`` holds the status word of every member inflated so far; with
    ``strict=False`` a member's status does not raise (its text is then undefined, that of the others is not)."""

    def __init__(self, path_or_bytes, device=None, batch_bytes=None, strict=True):
        _lib.require_gpu()
        from .counts import default_device
        self._handle = None
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            name, image = "<bytes>", path_or_bytes
        else:
            name = os.fspath(path_or_bytes)
            with open(name, "rb") as fh:
                image = fh.read()
        self._rec = _record(name, 'device')
        t0 = time.perf_counter()
        self._image = np.frombuffer(image, dtype=np.uint8)
        s = scan(self._image)
        self._rec['seconds']['scan'] = time.perf_counter() - t0
        self._rec['members'] = s['members']
        if s['status']:
            self._fail("member %d: %s" % (s['members'], _SCAN_STATUS[s['status']]))
        if s['members'] == 0:
            self._fail("an empty file")
        self._scan = s
        self._batch = BATCH_BYTES if batch_bytes is None else int(batch_bytes)
        device = default_device() if device is None else int(device)
        L = _lib.lib()
        self._handle = _lib.Handle("the BGZF inflater", lambda out: L.vrx_bgzf_create(device, self._batch, out),
                                   L.vrx_bgzf_destroy)
        self._next = 0                                  # first member of the next batch
        self._text, self._pos = np.zeros(0, np.uint8), 0
        self._strict = bool(strict)
        self.statuses = np.zeros(0, np.int32)

    def _fail(self, reason):
        self._rec.update(path='host', reason=reason)
        self.close()
        raise BgzfStatus(reason)

    def _inflate_batch(self):
        s, first = self._scan, self._next
        out_off = s['out_off']
        # as many members as fit the batch, one at least
        end = int(np.searchsorted(out_off, out_off[first] + self._batch, side='right')) - 1
        end = min(max(end, first + 1), s['members'])
        lo = int(s['payload_off'][first]) - 18
        hi = int(s['payload_off'][end - 1]) + int(s['payload_len'][end - 1]) + 8
        comp = self._image[lo:hi]
        poff = np.ascontiguousarray(s['payload_off'][first:end] - lo)
        plen = np.ascontiguousarray(s['payload_len'][first:end])
        ooff = np.ascontiguousarray(out_off[first:end + 1] - out_off[first])
        text = np.empty(int(ooff[-1]), np.uint8)
        status, sec = np.zeros(end - first, np.int32), np.zeros(3)
        _lib.check(_lib.lib().vrx_bgzf_inflate(
            self._handle.ptr, comp.ctypes.data_as(_lib._U8), len(comp), end - first, poff.ctypes.data_as(_lib._I64),
            plen.ctypes.data_as(_lib._I32), ooff.ctypes.data_as(_lib._I64),
            text.ctypes.data_as(_lib._U8) if len(text) else None, status.ctypes.data_as(_lib._I32), _lib.dptr(sec)))
        for k, v in zip(('upload', 'kernels', 'download'), sec):
            self._rec['seconds'][k] += float(v)
        self.statuses = np.concatenate([self.statuses, status])
        bad = np.flatnonzero(status)
        if len(bad) and self._strict:
            self._fail("member %d: %s" % (first + int(bad[0]), _member_reason(int(status[bad[0]]))))
        self._next = end
        self._text, self._pos = text, 0

    def read(self, n=-1):
        """up to n bytes of text (all that is left for n < 0); b'' at the end"""
        if self._handle is None:
            raise ValueError("read of a closed BgzfReader")
        if n is None or n < 0:
            parts = []
            while True:
                part = self.read(BATCH_BYTES)
                if not part:
                    return b"".join(parts)
                parts.append(part)
        while self._pos >= len(self._text) and self._next < self._scan['members']:
            self._inflate_batch()
        out = self._text[self._pos:self._pos + n].tobytes()
        self._pos += len(out)
        return out

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None
        self._text = np.zeros(0, np.uint8)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def inflate(path_or_bytes, device=None, batch_bytes=None):
    """The text of a BGZF file (a path, or the file's bytes): ``gzip.open(path).read()``, inflated on the device.
    Raises ``BgzfStatus`` for anything the device does not vouch for; there is no fallback here."""
    with BgzfReader(path_or_bytes, device, batch_bytes) as r:
        return r.read()
