"""Device buffers and option scopes shared by the kernel-against-fp64 GPU tests (test_gpu_conv.py,
test_gpu_trunk_edge.py): every output and workspace has exactly the advertised size, is pre-filled (NaN bit patterns,
zeros for counter words, or the values an in-place kernel starts from) and is followed by a guard block that ``check``
requires unchanged after the launch. Imported lazily-safe: nothing here touches the device until a method is called."""
import torch

BF = torch.bfloat16
GUARD = 256            # bytes after each output / workspace
GUARD_BYTE = 0xA5


class Bufs:
    """Exact-size device buffers, each followed by a guard block; ``check`` after the launch."""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def _new(self, nbytes, fill, zero):
        buf = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=self.dev)
        buf[nbytes:] = GUARD_BYTE
        self.all.append((buf, nbytes, zero))
        return buf

    def nan(self, shape, dtype):
        """A tensor of NaN bit patterns (0xFF bytes: a NaN in bf16 and in fp32) of exactly this shape."""
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * (2 if dtype == BF else 4)
        return self._new(nbytes, 0xFF, False)[:nbytes].view(dtype).view(shape)

    def ws(self, nbytes):
        """A workspace of exactly nbytes of NaN bit patterns; its data pointer (None for 0 bytes)."""
        return self._new(nbytes, 0xFF, False).data_ptr() if nbytes > 0 else None

    def zeros(self, nbytes):
        """Zeroed counter / claim words, which every launch must leave zero."""
        return self._new(nbytes, 0, True).data_ptr()

    def of(self, t):
        """An exact-size guarded copy of ``t`` (the operand an in-place or accumulating kernel updates)."""
        nbytes = t.numel() * t.element_size()
        out = self._new(nbytes, 0, False)[:nbytes].view(t.dtype).view(t.shape)
        out.copy_(t)
        return out

    def check(self):
        for buf, nbytes, zero in self.all:
            assert bool((buf[nbytes:] == GUARD_BYTE).all()), "the kernel wrote past a buffer"
            if zero:
                assert not bool(buf[:nbytes].any()), "counter words not left zero"


class opts:
    """``with opts([(name, value), ...])``: library options (csrc/common.h) set around a launch, restored after."""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from u3d import ops
        self.cms = [ops.option(k, v) for k, v in self.opts]
        for cm in self.cms:
            cm.__enter__()

    def __exit__(self, *a):
        for cm in reversed(self.cms):
            cm.__exit__(*a)


def ptr(t):
    return None if t is None else t.data_ptr()
