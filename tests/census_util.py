"""The launch census as a route check, shared by tests/test_gpu_views.py and tests/test_gpu_dirty_workspace.py: a case reads the
counts before and after its call and asserts that the kernel family it is meant for launched, so that a moved threshold fails the
case instead of re-routing it."""
import ctypes


def census(L):
    need = L.gf2_kernel_census(None, 0)
    buf = ctypes.create_string_buffer(need + 1)
    L.gf2_kernel_census(buf, need + 1)
    out = {}
    for ln in buf.value.decode().splitlines():
        parts = ln.split(None, 1)
        if len(parts) == 2 and parts[0].isdigit():
            out[parts[1].strip()] = out.get(parts[1].strip(), 0) + int(parts[0])
    return out


def assert_route(before, after, families):
    ran = sorted(k for k, v in after.items() if v > before.get(k, 0))
    for f in families:
        assert any(f in k for k in ran), "route check: no %s kernel ran (launched: %s)" % (f, ran)
