"""Device tickets (include/fsdp.h fsdp_submit_device): batches and results in the caller's GPU memory.

DeviceArray owns memory of a context's GPU; as_device_ptr accepts one, or any object that speaks ``__cuda_array_interface__``
(version 3: CuPy, torch on ROCm, ...).  The package itself imports no such framework.  A framework that bundles a HIP runtime
of its own (the torch wheels do) hands out pointers the runtime of this library does not know: the library refuses them
cleanly (FsdpError), see INTEGRATION.md.

DeviceFleet is n stateful planners stepped in lock-step, their previous paths kept on the device: one device ticket per tick,
nothing crosses PCIe, and the host waits for nothing between ticks.  SkidpadDeviceFleet is the same for the skidpad mission, whose
planners keep their state in the context (fsdp_skidpad_submit_device).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi


class DeviceArray:
    """A C-contiguous array in the memory of ``ctx``'s GPU (fsdp_device_alloc), freed by close() or with the object."""

    def __init__(self, ctx: "_capi.Context", shape, dtype=np.float64):
        self.ctx = ctx
        self.shape = tuple(int(x) for x in (shape if np.ndim(shape) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = ctx._lib.fsdp_device_alloc(ctx._h, ctypes.c_size_t(max(1, self.nbytes)))
        if not self.ptr:
            raise _capi.FsdpError(f"fsdp_device_alloc({self.nbytes}) failed")

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (int(self.ptr), False), "version": 3, "strides": None}

    def copy_from(self, host_array) -> "DeviceArray":
        """host -> device, synchronous; the array must have this one's shape (its dtype is converted)"""
        a = np.ascontiguousarray(host_array, dtype=self.dtype)
        if a.shape != self.shape:
            raise ValueError(f"copy_from: shape {a.shape}, this array is {self.shape}")
        self.ctx._check(self.ctx._lib.fsdp_device_write(self.ctx._h, ctypes.c_void_p(self.ptr), ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(self.nbytes)),
                        "fsdp_device_write")
        return self

    def numpy(self) -> np.ndarray:
        """device -> host, synchronous (on the context's own stream: wait for the ticket that writes the array first)"""
        out = np.empty(self.shape, self.dtype)
        self.ctx._check(self.ctx._lib.fsdp_device_read(self.ctx._h, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(self.ptr), ctypes.c_size_t(self.nbytes)),
                        "fsdp_device_read")
        return out

    def close(self):
        if getattr(self, "ptr", None) and getattr(self.ctx, "_h", None):
            self.ctx._lib.fsdp_device_free(self.ctx._h, ctypes.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_array(ctx, host_array, dtype=None) -> DeviceArray:
    """A DeviceArray holding a copy of ``host_array``."""
    a = np.ascontiguousarray(host_array, dtype=dtype)
    return DeviceArray(ctx, a.shape, a.dtype).copy_from(a)


def as_device_ptr(obj, shape, dtype, writable: bool = False) -> int:
    """The device address of ``obj`` — a DeviceArray or any object with ``__cuda_array_interface__`` — after checking shape, dtype
    and C-contiguity, and, for an array the library writes (``writable``), that the interface does not mark it read-only.  A NumPy
    array (host memory) is a TypeError: it goes through Context.submit.  The interface's optional ``stream`` entry is NOT
    honoured: nothing is synchronised here, the caller orders the library behind the array's producer with ``after_stream``
    (Context.submit_device) or hands over arrays that are complete."""
    if isinstance(obj, np.ndarray) or not hasattr(obj, "__cuda_array_interface__"):
        raise TypeError(f"{type(obj).__name__} is no device array (__cuda_array_interface__); host arrays go through Context.submit")
    cai = obj.__cuda_array_interface__
    shape, dtype = tuple(int(x) for x in shape), np.dtype(dtype)
    if tuple(cai["shape"]) != shape:
        raise ValueError(f"device array of shape {tuple(cai['shape'])}, expected {shape}")
    got = np.dtype(cai["typestr"])
    # (an array of records — the interface's typestr knows them only as opaque items, '|V32' — matches by its item size)
    if got != dtype and not (dtype.fields is not None and got.kind == "V" and got.itemsize == dtype.itemsize):
        raise ValueError(f"device array of dtype {got}, expected {dtype}")
    strides = cai.get("strides")
    if strides is not None:
        want, acc = [], dtype.itemsize
        for extent in reversed(shape):
            want.append(acc)
            acc *= extent
        if any(e > 1 and s != w for e, s, w in zip(shape, strides, reversed(want))):
            raise ValueError(f"device array is not C-contiguous (strides {tuple(strides)})")
    ptr, read_only = cai["data"][0], bool(cai["data"][1])
    if writable and read_only:
        raise ValueError("device array is read-only, and the library writes this one")
    if not ptr and int(np.prod(shape, dtype=np.int64)) > 0:
        raise ValueError("device array with a NULL pointer")
    return int(ptr)


class DeviceTicket(_capi.Ticket):
    """A device ticket in flight (Context.submit_device); ``out`` is the dict of device arrays collect() returns."""

    __slots__ = ()


class DeviceFleet:
    """n_planners stateful planners stepped in lock-step with their previous paths kept on the device.

    step() submits one device ticket with prev = next_prev = the fleet's buffer, ordered behind the fleet's previous step on a
    stream the fleet owns (fsdp_ticket_stream_wait), and returns at once: (paths, status, ticket), the first two device arrays
    that are final once the ticket is done (Context.stream_wait(ticket, consumer_stream), or fleet.wait()).  At most
    ``ctx.ticket_capacity`` (2 x depth) steps are outstanding: a further step first collects the oldest one."""

    def __init__(self, n_planners: int, cone_capacity: int, mission=None, params: dict | None = None, device: int | None = None, depth: int = 2,
                 ctx: "_capi.Context | None" = None):
        from .planner import MissionTypes

        mission = MissionTypes.trackdrive if mission is None else mission
        self.n, self.cap = int(n_planners), int(cone_capacity)
        if self.n < 1 or self.cap < 0:
            raise ValueError("DeviceFleet: n_planners >= 1 and cone_capacity >= 0")
        self._own_ctx = ctx is None
        self.ctx = _capi.Context(device=device, mission=int(mission), params=params) if ctx is None else ctx
        if self._own_ctx:
            self.ctx.set_overlap(int(depth))
        self._stream = self.ctx.stream_create()
        self._prev = DeviceArray(self.ctx, (self.n, self.ctx.shapes.path_points, 4))
        self._tickets: list = []
        self.reset()

    def reset(self, initial_prev=None):
        """Fresh planners (the context's default path), or planners that start from ``initial_prev`` (n, <= path_points, 4)."""
        self.wait()
        rows = np.broadcast_to(self.ctx.default_path(), self._prev.shape) if initial_prev is None else self.ctx.pad_paths(initial_prev)
        self._prev.copy_from(rows)

    def step(self, counts, cones, poses, after_stream=None, paths=None, status=None, path_ids=None):
        """One tick: counts (n) int32, cones (n, cone_capacity, 3) or None when cone_capacity = 0, poses (n, 4) — device arrays.
        after_stream: the stream that produces them (a hipStream_t as an int), or None when they are complete.
        path_ids: a device (n) int32 array — planner i follows entry path_ids[i] of the context's path table
        (Context.set_global_path_table) in this tick, or plans from its cones with -1; its previous path travels across a switch."""
        ctx = self.ctx
        while len(self._tickets) >= ctx.ticket_capacity:
            ctx.collect(self._tickets.pop(0))
        if self._tickets:
            ctx.stream_wait(self._tickets[-1], self._stream)  # (behind the step that writes the previous paths this one reads)
        if after_stream is not None:
            ctx.stream_wait_stream(self._stream, after_stream)
        t = ctx.submit_device(counts, cones, poses, prev=self._prev, paths=paths, status=status, next_prev=self._prev, after_stream=self._stream,
                              cone_capacity=self.cap, path_ids=path_ids)
        self._tickets.append(t)
        return t.out["paths"], t.out["status"], t

    def wait(self):
        """Collect every outstanding step (raises FsdpError for a step with a count out of range)."""
        err = None
        while self._tickets:
            try:
                self.ctx.collect(self._tickets.pop(0))
            except _capi.FsdpError as e:
                err = err or e
        if err is not None:
            raise err

    def previous_paths(self) -> np.ndarray:
        """The planners' previous paths (n, path_points, 4) as a host copy; waits for every outstanding step."""
        self.wait()
        return self._prev.numpy()

    def close(self):
        if getattr(self, "ctx", None) is None:
            return
        try:
            self.wait()
        finally:
            if self._stream:
                self.ctx.stream_destroy(self._stream)
                self._stream = None
            self._prev.close()
            if self._own_ctx:
                self.ctx.close()
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SkidpadDeviceFleet:
    """n_planners skidpad planners stepped in a closed loop on the GPU (SkidpadBatch.submit_device): one device ticket per tick.

    The planners' state — latch, transform, window index, previous path — lives in the context, and all skidpad work runs on the
    context's one stream in submit order, so consecutive steps need no ordering from the fleet.  step() returns at once: (paths,
    status, ticket), the first two device arrays that are final once the ticket is done (``ctx.stream_wait(ticket,
    consumer_stream)``, or fleet.wait()).  At most ``depth`` steps are outstanding: a further step first collects the oldest one.
    A ``reset`` mask (n) int32 on the device restarts single planners in front of a step; reset() restarts all of them."""

    def __init__(self, n_planners: int, cone_capacity: int, device: int | None = None, params: dict | None = None, depth: int = 4,
                 table=None):
        from .skidpad import SkidpadBatch

        self.n, self.cap = int(n_planners), int(cone_capacity)
        if self.n < 1 or self.cap < 0:
            raise ValueError("SkidpadDeviceFleet: n_planners >= 1 and cone_capacity >= 0")
        self.batch = SkidpadBatch(self.n, device=device, table=table, params=params)
        self.ctx = self.batch._ctx
        self.batch.set_overlap(int(depth))
        self._tickets: list = []

    def step(self, counts, cones, poses, reset=None, after_stream=None, paths=None, status=None, info=None):
        """One tick: counts (n) int32, cones (n, cone_capacity, 3) or None when cone_capacity = 0, poses (n, 4), reset (n) int32 or
        None — device arrays.  after_stream: the stream that produces them (a hipStream_t as an int), or None when they are
        complete.  info: True or a device array of INFO_DTYPE records (ticket.out["info"])."""
        while len(self._tickets) >= self.ctx.ticket_capacity:
            self.batch.collect(self._tickets.pop(0))
        t = self.batch.submit_device(counts, cones, poses, reset=reset, paths=paths, status=status, info=info, after_stream=after_stream,
                                     cone_capacity=self.cap)
        self._tickets.append(t)
        return t.out["paths"], t.out["status"], t

    def wait(self):
        """Collect every outstanding step (raises FsdpError for a step with a count out of range)."""
        err = None
        while self._tickets:
            try:
                self.batch.collect(self._tickets.pop(0))
            except _capi.FsdpError as e:
                err = err or e
        if err is not None:
            raise err

    def reset(self):
        """Fresh planners, all of them (fsdp_skidpad_reset: the host call, which waits for every outstanding step)."""
        try:
            self.wait()
        finally:
            self.batch.reset()

    def close(self):
        if getattr(self, "batch", None) is None:
            return
        try:
            self.wait()
        finally:
            self.batch.close()
            self.batch = self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
