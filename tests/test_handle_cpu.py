"""The Python owner of a library handle (``_lib.Handle``), driven with recording fakes in place of
``vrx_X_create`` and ``vrx_X_destroy``: no library call that touches a device, no GPU."""
import gc

import pytest

from vireo_amd import _lib


class Fakes:
    """create hands out the pointers 1, 2, ... and destroy records which pointer it was given, in order"""

    def __init__(self, status=0):
        self.status, self.made, self.destroyed = status, 0, []

    def create(self, out):
        if self.status == 0:
            self.made += 1
            out._obj.value = self.made
        return self.status

    def destroy(self, ptr):
        self.destroyed.append(ptr.value)


def test_destroy_runs_exactly_once():
    f = Fakes()
    h = _lib.Handle("fake", f.create, f.destroy)
    assert h.ptr.value == 1 and h._h is h.ptr and f.destroyed == []
    h.close()
    assert f.destroyed == [1]
    h.close()
    del h
    gc.collect()
    assert f.destroyed == [1]


def test_collection_destroys_an_open_handle():
    f = Fakes()
    h = _lib.Handle("fake", f.create, f.destroy)
    del h
    gc.collect()
    assert f.destroyed == [1]


def test_failed_create_registers_no_destroy(monkeypatch):
    class Lib:
        @staticmethod
        def vrx_last_error():
            return b"fake: no such thing"

    monkeypatch.setattr(_lib, "_lib", Lib)              # (check() asks the library for the message)
    f = Fakes(status=2)
    with pytest.raises(_lib.VrxError, match="no such thing"):
        _lib.Handle("fake", f.create, f.destroy)
    gc.collect()
    assert f.made == 0 and f.destroyed == []


def test_pointer_after_close_raises():
    f = Fakes()
    h = _lib.Handle("the fake table", f.create, f.destroy)
    h.close()
    for name in ("ptr", "_h"):
        with pytest.raises(_lib.VrxError, match="the fake table is closed"):
            getattr(h, name)


def test_context_manager_closes_on_exit_and_on_exception():
    f = Fakes()
    with _lib.Handle("fake", f.create, f.destroy) as h:
        assert h.ptr.value == 1 and f.destroyed == []
    assert f.destroyed == [1]
    with pytest.raises(KeyError):
        with _lib.Handle("fake", f.create, f.destroy) as h:
            raise KeyError("inside")
    assert f.destroyed == [1, 2]
    with pytest.raises(_lib.VrxError):
        h.ptr


def test_kept_parent_outlives_its_child_in_one_collection():
    """a child and the parent it keeps die in one cycle: the child is destroyed first"""
    f = Fakes()
    parent = _lib.Handle("parent", f.create, f.destroy)
    child = _lib.Handle("child", f.create, f.destroy, keep=(parent,))
    assert (parent.ptr.value, child.ptr.value) == (1, 2)
    ring = [parent, child]                                # (the parent first: no order of the list helps)
    ring.append(ring)
    gc.collect()
    del parent, child, ring
    gc.collect()
    assert f.destroyed == [2, 1]
