"""Host threads and the Python package's lazily created objects, without a GPU: ``Workspace``, ``Plan`` and the loader
of the library are replaced by slow stubs (``monkeypatch``), so that threads really race on first use.

* ``default_workspace()`` is per (thread, device) - the reference's thread-local CACHE (src/lib.rs:217-219), like
  ``Workspace::thread_default()`` of the C++ mirror: two threads in one workspace would run inside the same device
  buffers at once (the library holds no lock on a workspace, and ctypes releases the GIL for the whole call);
* ``Builder.plan()`` / ``text_plan()`` and ``lib()`` create one object however many threads race on them.
"""
import sys
import threading
import time

N_THREADS = 8


def _race(fn, n=N_THREADS):
    """fn(i) in n threads released together; their results in thread order (raises the first exception)."""
    barrier = threading.Barrier(n)
    out, errs = [None] * n, []

    def body(i):
        try:
            barrier.wait()
            out[i] = fn(i)
        except BaseException as e:  # (re-raised in the main thread)
            errs.append(e)

    threads = [threading.Thread(target=body, args=(i,)) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    return out


class _SlowCounter:
    """Constructor stand-in that counts instances and sleeps (without the GIL) while it 'creates' one."""

    def __init__(self):
        self.made = []
        self.lock = threading.Lock()

    def make(self, *args, **kwargs):
        time.sleep(0.05)
        obj = type("Stub", (), {})()
        obj.args, obj.kwargs = args, kwargs
        with self.lock:
            self.made.append(obj)
        return obj


def test_default_workspace_per_thread_and_device(sm, monkeypatch):
    counter = _SlowCounter()
    monkeypatch.setattr(sm, "Workspace", counter.make)
    monkeypatch.setitem(sys.modules, "torch", None)  # (no torch stream to bind: the stub gets stream=None)

    def body(i):
        a0 = sm.default_workspace(0)
        a1 = sm.default_workspace(1)
        return a0, a1, sm.default_workspace(0), sm.default_workspace(1)

    res = _race(body)
    for a0, a1, b0, b1 in res:
        assert a0 is b0 and a1 is b1  # stable within a thread
        assert a0 is not a1
        assert a0.args == (0, None) and a1.args == (1, None)
    firsts = [id(r[0]) for r in res] + [id(r[1]) for r in res]
    assert len(set(firsts)) == 2 * N_THREADS, "threads share a default workspace"
    assert len(counter.made) == 2 * N_THREADS


def test_default_workspace_not_inherited_from_a_finished_thread(sm, monkeypatch):
    """A thread's workspace is its own: one created by another (now finished) thread is never handed out."""
    counter = _SlowCounter()
    monkeypatch.setattr(sm, "Workspace", counter.make)
    monkeypatch.setitem(sys.modules, "torch", None)
    first = _race(lambda i: sm.default_workspace(0), n=1)[0]
    second = _race(lambda i: sm.default_workspace(0), n=1)[0]
    assert first is not second and len(counter.made) == 2


def test_lazy_plans_created_once(sm, monkeypatch):
    counter = _SlowCounter()
    monkeypatch.setattr(sm, "Plan", counter.make)
    b = sm.canonical_minimizers(21, 11)
    plans = _race(lambda i: b.plan())
    assert len(counter.made) == 1 and all(p is plans[0] for p in plans)
    assert plans[0].args == (21, 11, True, sm.MM_MINIMIZERS, None)
    text_plans = _race(lambda i: b.text_plan())
    assert len(counter.made) == 2 and all(p is text_plans[0] for p in text_plans)
    assert text_plans[0] is not plans[0] and text_plans[0].kwargs == {"text": True}
    # both kinds at once on a fresh builder
    b2 = sm.minimizers(5, 7)
    mixed = _race(lambda i: b2.plan() if i % 2 else b2.text_plan())
    assert len(counter.made) == 4
    assert all(p is b2.plan() for p in mixed[1::2]) and all(p is b2.text_plan() for p in mixed[0::2])


class _FakeFunction:
    pass


class _FakeLib:
    """What the loader sees of a CDLL: any symbol, with settable argtypes / restype."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        f = _FakeFunction()
        setattr(self, name, f)
        return f


def test_lib_loaded_once(sm, monkeypatch):
    counter = _SlowCounter()

    def cdll(path):
        counter.make(path)
        return _FakeLib()

    monkeypatch.setattr(sm, "_lib", None)
    monkeypatch.setattr(sm, "LIB_PATH", __file__)  # (an existing file: the stub never opens it)
    monkeypatch.setattr(sm.C, "CDLL", cdll)
    libs = _race(lambda i: sm.lib())
    assert len(counter.made) == 1, f"{len(counter.made)} loads of the library"
    assert all(L is libs[0] for L in libs) and isinstance(libs[0], _FakeLib)
    assert libs[0].mm_last_error.restype is sm.C.c_char_p  # bound before any thread saw it

