"""What the per-form GPU test modules share: failures collected per case (a HIP runtime error ends the module at once: nothing more is
started on a device that may have faulted), and outputs placed inside 0xFF-filled allocations whose guard bytes must come back untouched."""
import math

import pytest
import torch


class Failures:
    def __init__(self):
        self.items = []

    def run(self, what, fn):
        try:
            return fn()
        except AssertionError as e:
            self.items.append(f"{what}: {e}")
        except RuntimeError as e:
            # a failed launch (the library's error -2) or an error the HIP runtime reports ends the module: nothing more is started on a device
            # that may have faulted.  Anything else - a refusal by the library (bad argument, unsupported form), a shape or dtype error of the
            # test's own torch code - is one failing case, once the device has answered a synchronize
            msg = str(e)
            if ("libudapose_hip call failed" in msg and "error -2" in msg) or any(k in msg for k in ("HIP error", "hipError", "CUDA error")):
                pytest.exit(f"GPU runtime failure in {what}: {e}", returncode=3)
            try:
                torch.cuda.synchronize()
            except RuntimeError as e2:
                pytest.exit(f"GPU runtime failure after {what}: {e2}", returncode=3)
            self.items.append(f"{what}: {type(e).__name__}: {e}")
        return None

    def assert_none(self):
        assert not self.items, f"{len(self.items)} failing form(s):\n" + "\n".join(self.items[:40])


class Guards:
    """Outputs as views inside 0xFF-filled allocations; check() asserts that every guard is untouched."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype, row, init=None):
        item = torch.empty((), dtype=dtype).element_size()
        n = math.prod(shape) * item
        g = max(256, -(-row * item // 256) * 256)
        buf = torch.full((n + 2 * g,), 0xFF, dtype=torch.uint8, device="cuda")
        self.items.append((buf, g, n))
        v = buf[g:g + n].view(dtype).view(shape)
        if init is not None:
            v.copy_(init)
        return v

    def check(self, what):
        bad = [i for i, (buf, g, n) in enumerate(self.items) if not (bool((buf[:g] == 0xFF).all()) and bool((buf[g + n:] == 0xFF).all()))]
        self.items = []
        assert not bad, f"{what}: guard bytes around output(s) {bad} were overwritten"
