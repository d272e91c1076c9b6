"""What every streaming driver shares on the host: the window plan of forward_chunk_by_chunk and the hipGraph capture recipe
(warm up on a side stream, capture one step, replay it; stay eager only where the runtime refused the capture).  Callers keep
their own fixed buffers and their own replay loops."""
from typing import Callable, List, Optional, Tuple

import torch


def chunk_windows(embed, decoding_chunk_size: int, T: int) -> Tuple[List[int], int, int]:
    """(starts, window, stride) of a T-frame utterance cut as forward_chunk_by_chunk cuts it (wenet/transformer/encoder.py:
    379-391): a window of (chunk - 1) * subsampling + right_context + 1 input frames every subsampling * chunk frames, as
    long as a window's first output frame fits (the last window may be shorter: slice to min(start + window, T))."""
    sub, ctx = embed.subsampling_rate, embed.right_context + 1
    stride, window = sub * decoding_chunk_size, (decoding_chunk_size - 1) * sub + ctx
    return list(range(0, T - ctx + 1, stride)), window, stride


def capture_refused(e: BaseException) -> bool:
    """Is this the runtime refusing an operation under stream capture (hipErrorStreamCapture* -- a synchronising call, an
    allocation the graph pool cannot serve, a capture-unsafe library call), as opposed to an error of the work itself?"""
    from .._lib import PafcError
    if isinstance(e, PafcError):
        return False
    msg = str(e).lower()
    return "captur" in msg


def abandon_capture(device) -> None:
    """After a capture the runtime refused: let the device drain, taking the runtime's echo of the error here (an invalidated
    capture reports itself once more through the next synchronising call) rather than in the caller's next unrelated operation.
    Best effort: on ROCm 7.0's HIP inside torch 2.10 an invalidated capture keeps failing every later call of the process with
    hipErrorStreamCaptureInvalidated -- ending the capture on its stream by hand (hipStreamEndCapture + hipGetLastError through
    ctypes) was tried in round 6 and changes nothing, and is not done here: a second copy of the HIP runtime could get loaded for
    it.  tests/test_encoder_gpu.py::test_refused_capture_is_never_silent_in_a_child_process records which way a runtime
    behaves; what cannot be cleared surfaces at the caller's next call, naming the capture."""
    for _ in range(2):
        try:
            torch.cuda.synchronize(device)
            break
        except RuntimeError as again:
            if not capture_refused(again):
                raise


_SIDE_STREAMS = {}


def side_stream(device) -> torch.cuda.Stream:
    """The side stream warm-ups (and the captures that ask for it) run on: one per device, as torch.cuda.graph keeps one of
    its own."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _SIDE_STREAMS:
        _SIDE_STREAMS[idx] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[idx]


def on_side_stream(device, fn: Callable):
    """fn() on the device's side stream, forked from and joined to the current stream: the eager steps before a capture, which
    warm every kernel and library handle up where torch.cuda.graph wants them (off the default stream).  Returns fn()."""
    side, main = side_stream(device), torch.cuda.current_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    main.wait_stream(side)
    return out


def capture(fn: Callable, device, stream: Optional[torch.cuda.Stream] = None) -> Tuple[Optional[torch.cuda.CUDAGraph], object]:
    """Capture fn() into a hipGraph (on `stream` when given, else on torch.cuda.graph's own) -> (graph, what fn returned: the
    graph's static outputs).  A capture the runtime REFUSES (capture_refused) gives (None, None) after abandon_capture:
    nothing ran, so the caller's state is as before and it goes on eagerly.  Every other error -- a failing launch, a
    PafcError -- is an error of the work and propagates."""
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=stream):
            out = fn()
    except RuntimeError as e:
        if not capture_refused(e):
            raise
        abandon_capture(device)
        return None, None
    return graph, out
