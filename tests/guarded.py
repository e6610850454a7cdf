"""NaN-guarded device buffers for the kernel-level GPU tests (TEST INFRASTRUCTURE - a plain helper module).

A kernel's output (or an input it must leave alone) lives inside a larger allocation filled with NaN: padding columns behind every row and
guard rows on both sides. After the call everything but the payload must come back bit for bit untouched, and the payload finite."""
import torch

bf16 = torch.bfloat16
GUARD = 64


def _dev():
    return torch.device("cuda:0")


class Guarded:
    """[guard + rows + guard][ld] bf16 on the device, NaN everywhere; the payload is rows x C at row `guard`."""

    def __init__(self, rows, C, ld=None, guard=GUARD, data=None):
        self.rows, self.C, self.ld, self.guard = rows, C, ld or C, guard
        assert self.ld >= C
        self.buf = torch.full((rows + 2 * guard, self.ld), float("nan"), dtype=bf16, device=_dev())
        if data is not None:
            self.payload.copy_(data.reshape(rows, C).to(_dev()))

    @property
    def payload(self):
        return self.buf[self.guard:self.guard + self.rows, :self.C]

    @property
    def ptr(self):
        return self.buf[self.guard:].data_ptr()

    def ptr_at(self, elements):
        """address `elements` bf16 values past the payload's start (for deliberately offset bases)"""
        return self.ptr + 2 * elements

    def assert_only_payload_written(self, what):
        fill = torch.full((1,), float("nan"), dtype=bf16, device=self.buf.device).view(torch.int16)
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[self.guard:self.guard + self.rows, :self.C] = False
        touched = int((self.buf.view(torch.int16)[outside] != fill).sum())
        assert touched == 0, f"{what}: {touched} elements of the guard rows / padding columns were written"
        assert bool(torch.isfinite(self.payload.float()).all()), f"{what}: non-finite values in the payload"

    def cpu(self):
        return self.payload.cpu()
