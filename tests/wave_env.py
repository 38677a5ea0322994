"""What the GPU tests of the wavefront pipelines' switches share (test_gpu_primary_reuse.py, test_gpu_shadow_reuse.py,
test_gpu_dead_shadow.py, test_gpu_dead_brdf.py, test_gpu_deferred_resolve.py): environment switches around a block of
calls, and a handful of contexts that are closed behind it."""
import contextlib

import prt


@contextlib.contextmanager
def env(monkeypatch, **kv):
    """Environment switches for the calls inside the block (the library reads them per call)."""
    for k, v in kv.items():
        monkeypatch.setenv(k, v)
    try:
        yield
    finally:
        for k in kv:
            monkeypatch.delenv(k, raising=False)


@contextlib.contextmanager
def env_or_unset(monkeypatch, **kv):
    """Environment switches for the calls inside the block (the library reads them per call); None leaves unset."""
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    try:
        yield
    finally:
        for k in kv:
            monkeypatch.delenv(k, raising=False)


@contextlib.contextmanager
def contexts(n):
    cs = [prt.Context(0) for _ in range(n)]
    try:
        yield cs
    finally:
        for c in cs:
            c.close()
