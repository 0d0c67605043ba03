"""What integral.py and made.py share on the way to a native call: the graph-mode predicate, tensor addresses that refuse
torch.jit.trace, and the current stream."""
import ctypes
import sys

import torch


def _graph_mode():
    """True while torch.compile / torch.export trace a call (Dynamo) or torch.jit.trace records one: the HIP launches then
    go through the ``torch.ops.umnn`` ops (ops.py), which the graph records, instead of ctypes calls it cannot see."""
    return torch.compiler.is_compiling() or torch.jit.is_tracing()


def traced_native_call():
    """The error for a native pointer taken while torch.jit.trace records: the tracer would keep the output allocation and
    drop the launch, so the traced graph would return uninitialised memory.  Names the function that took the pointer."""
    fn = sys._getframe(2).f_code.co_name
    return RuntimeError(f"umnn_amd: {fn}() passed a tensor to a native call while torch.jit.trace was recording; the trace "
                        "would not contain that launch.  Traced code has to reach the HIP kernels through torch.ops.umnn "
                        "(umnn_amd.ops).")


def _address(t):
    """data_ptr() for a native call (what a ctypes struct field takes); raises under torch.jit.trace."""
    if torch._C._is_tracing():
        raise traced_native_call()
    return t.data_ptr()


def _ptr(t):
    """``_address`` as a ctypes argument; None stays None (a null pointer)."""
    if t is None:
        return None
    if torch._C._is_tracing():
        raise traced_native_call()
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
