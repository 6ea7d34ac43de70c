"""What the drop-in envs' step servers share on the host (include/scgpu.h scg_bg_server_*,
scg_sc_server_*; the C side of the same lifecycle is csrc/scg_server_host.h): a non-blocking
stream of the device's highest priority, the mailbox in host-mapped memory, stop() and
close(), and one registry that closes every server at interpreter exit. beergame_env's
_StepServer adds slots and their sharing, supplychain_env's _ScStepServer its step().
"""
import atexit
import ctypes
import weakref

import torch

from .. import _native as nat
from . import resident

_LIVE = weakref.WeakSet()  # every server not yet closed


@atexit.register
def _close_servers():  # no resident wave or block outlives the interpreter (nor its mailbox)
    for server in list(_LIVE):
        server.close()


class _ResidentServer:
    """One resident wave or block polling a mailbox. A subclass sets `sv`, the C server struct
    (box_host, box_dev and stream from `box_addrs` and `stream`). The wave exits when stopped
    (close(), another server of the device becoming resident, interpreter exit) or by itself
    after IDLE_US without a request; a post launches it again when needed. The mailbox is
    freed only after the wave has been stopped."""

    IDLE_US = 20000

    def __init__(self, device, dev_index, box_type, stop_fn):
        self._device, self._dev_index, self._stop_fn = device, dev_index, stop_fn
        self._closed = True  # until every part exists (a half-built server closes as a no-op)
        self.stream, self.priority = resident.server_stream(device)
        self._box = box = nat.MappedBuffer(ctypes.sizeof(box_type))
        self.box = box_type.from_address(box.host)
        self.box_addrs = (box.host, box.dev)
        self.sv = None
        self._closed = False
        _LIVE.add(self)

    @property
    def launches(self):
        return int(self.sv.launches)

    def stop(self):
        if not self._closed and self.sv is not None:
            with torch.cuda.device(self._device):
                nat.check(self._stop_fn(ctypes.byref(self.sv)))

    def close(self):
        if self._closed:
            return
        self.stop()  # raises if the wave cannot be stopped: then the mailbox stays allocated
        self._closed = True
        resident.release(self._dev_index, self)
        resident.destroy_stream(self.stream)
        self.box = self._box = None
        _LIVE.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter teardown
            pass
