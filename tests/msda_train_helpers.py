"""Helpers of the msda_train tests: the launch-form record of csrc/msda_train.hip and the host evaluation through ctypes."""
import contextlib
import ctypes

import numpy as np
import torch


@contextlib.contextmanager
def msda_train_served_by(forms):
    """As helpers.msda_served_by for the record of msda_train.hip (lwdetr_msda_train_path_counts): the lwdetr_msda_train_forward / _backward
    launches inside the block went to exactly the instantiations `forms` ({name of lwdetr_msda_train_path_name: launches}), and to no other."""
    from lwdetr_amd import _native
    before = _native.msda_train_path_counts()
    for f in forms:
        assert f in before, f"unknown msda_train kernel form {f!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.msda_train_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert delta == dict(forms), f"launch forms {delta}, expected {dict(forms)}"


def host_backward(native, inp):
    """lwdetr_msda_train_backward_host on every (row, head) of a case (inputs widened to f32): grad_value / grad_ref summed by the entry itself,
    rows and heads in order. -> dict of float32 tensors named as msda_train_ref.TENSORS without `out`."""
    case = inp["case"]
    B, Q, M, D, P = case["B"], case["Q"], case["M"], case["D"], case["P"]
    L, S = inp["shapes"].shape[0], inp["S"]
    f = lambda t: np.ascontiguousarray(t.float().numpy())
    value, off, lg, go, ref = f(inp["value"]), f(inp["off"]), f(inp["lg"]), f(inp["go"]), f(inp["ref"])
    mask = None if inp["mask"] is None else np.ascontiguousarray(inp["mask"].numpy().astype(np.uint8))
    shapes, lsi = np.ascontiguousarray(inp["shapes"].numpy()), np.ascontiguousarray(inp["lsi"].numpy())
    gv, g_off, g_lg, g_ref = np.zeros_like(value), np.zeros_like(off), np.zeros_like(lg), np.zeros_like(ref)
    fn = native.lib().lwdetr_msda_train_backward_host
    a = lambda arr, byte_off=0: ctypes.c_void_p(arr.ctypes.data + byte_off)
    LP = L * P
    for b in range(B):
        for q in range(Q):
            for m in range(M):
                vo = ((b * S) * M + m) * D * 4
                rm = ((b * Q + q) * M + m)
                rc = fn(a(value, vo), M * D, None if mask is None else a(mask, b * S), a(shapes), a(lsi), D, L, P, a(off, rm * LP * 8), a(lg, rm * LP * 4),
                        a(ref, (b * Q + q) * L * 16), a(go, rm * D * 4), a(gv, vo), M * D, a(g_off, rm * LP * 8), a(g_lg, rm * LP * 4),
                        a(g_ref, (b * Q + q) * L * 16))
                assert rc == 0, rc
    return dict(grad_value=torch.from_numpy(gv), grad_offsets=torch.from_numpy(g_off), grad_logits=torch.from_numpy(g_lg),
                grad_ref=torch.from_numpy(g_ref))
