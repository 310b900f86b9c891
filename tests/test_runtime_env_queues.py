"""lvk_runtime_env and GPU_MAX_HW_QUEUES (include/lvk_c.h, larvio_amd/csrc/lvk_context.hip): an explicit call with LVK_RT_HW_QUEUES raises
a preset number below 8 to 8 and reports the flag; 8 or more is left alone; the implicit call of lvk_context_create never overrides a
variable the user has set.  No GPU is needed: the environment is settled before the process's first HIP call, and each case runs in
a child process of its own that only loads the library (the environment is process-wide state, read once by the runtime)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVK_RT_HW_QUEUES = 1

_CHILD = """
import ctypes, os, sys
so = os.environ.get("LVK_LIB", os.path.join(%r, "larvio_amd", "liblvk_hip.so"))
L = ctypes.CDLL(so)
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p; libc.getenv.argtypes = [ctypes.c_char_p]
L.lvk_runtime_env.restype = ctypes.c_uint; L.lvk_runtime_env.argtypes = [ctypes.c_uint, ctypes.c_int]
if sys.argv[1] == "explicit":
    done = L.lvk_runtime_env(1, 0)
else:                                   # the LVK_RT_DEFAULT route: lvk_context_create applies it by itself, whether or not a device is there
    h = ctypes.c_void_p()
    L.lvk_context_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    if L.lvk_context_create(0, ctypes.byref(h)) == 0:
        L.lvk_context_destroy.argtypes = [ctypes.c_void_p]; L.lvk_context_destroy(h)
    done = 0
v = libc.getenv(b"GPU_MAX_HW_QUEUES")
print("RESULT", done, v.decode() if v is not None else "unset")
"""


@pytest.mark.parametrize("preset,route,value,reported", [("4", "explicit", "8", True), ("16", "explicit", "16", False), (None, "explicit", "8", True),
                                                         ("4", "default", "4", False)])
def test_hw_queues_request(preset, route, value, reported):
    env = dict(os.environ)
    env.pop("GPU_MAX_HW_QUEUES", None); env.pop("LVK_RUNTIME_ENV", None); env.pop("LVK_RUNTIME_BIND", None)
    if preset is not None:
        env["GPU_MAX_HW_QUEUES"] = preset
    p = subprocess.run([sys.executable, "-c", _CHILD % ROOT, route], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert line[2] == value, p.stdout
    assert bool(int(line[1]) & LVK_RT_HW_QUEUES) == reported, p.stdout
