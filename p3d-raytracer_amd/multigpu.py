"""One process per GPU: the stripes of a frame a rank renders, and the gather that puts them together (torch.distributed
moves the bytes; torch is imported where it is needed)."""
import numpy as np

from ._abi import Tile


def stripe_tile(res, rank, world, stripe_h=16):
    """Tile of rank `rank` in an N-rank job: every world-th stripe of stripe_h rows (DESIGN.md multi-GPU).
    Requires res_y % (stripe_h * world) == 0 so that every rank renders the same number of rows."""
    rx, ry = res
    if ry % (stripe_h * world) != 0:
        raise ValueError("res_y=%d must be a multiple of stripe_h*world=%d" % (ry, stripe_h * world))
    return Tile(0, rank * stripe_h, rx, ry // world, stripe_h, world)


def stripe_rows(res, rank, world, stripe_h=16):
    """Image rows (bottom-up numbering) that `stripe_tile` renders, in local-row order."""
    t = stripe_tile(res, rank, world, stripe_h)
    r = np.arange(t.h)
    return t.y0 + (r // stripe_h) * stripe_h * world + (r % stripe_h)


# ---- multi-GPU helpers (one process per GPU; torch.distributed moves the bytes) ----
def packed_bytes(n_pixels):
    """Per-rank framebuffer layout used for the gather: [rgb float32 x3 | hit int32] = 16 B/pixel."""
    return n_pixels * 16


def assemble_frame(gathered, res, world, stripe_h, frame_rgb=None, frame_hit=None, batch=1):
    """De-interleave the per-rank stripe buffers (torch uint8 tensors, `batch` consecutive frames each
    laid out as packed_bytes) into full frames: stripe s of rank r holds frame rows
    (s*world + r)*stripe_h ... +stripe_h.  Returns (rgb, hit) of shape (ry, rx, 3) / (ry, rx), with a
    leading batch axis when batch > 1."""
    import torch
    rx, ry = res
    n_str = ry // (stripe_h * world)
    n_local = rx * (ry // world)
    dev = gathered[0].device
    if frame_rgb is None:
        frame_rgb = torch.empty((batch, ry, rx, 3), dtype=torch.float32, device=dev)
    if frame_hit is None:
        frame_hit = torch.empty((batch, ry, rx), dtype=torch.int32, device=dev)
    per_frame = [g.view(batch, n_local * 16) for g in gathered]
    parts = [g[:, : n_local * 12].contiguous().view(torch.float32).view(batch, n_str, stripe_h, rx, 3) for g in per_frame]
    frame_rgb.view(batch, n_str, world, stripe_h, rx, 3).copy_(torch.stack(parts, dim=2))
    hits = [g[:, n_local * 12:].contiguous().view(torch.int32).view(batch, n_str, stripe_h, rx) for g in per_frame]
    frame_hit.view(batch, n_str, world, stripe_h, rx).copy_(torch.stack(hits, dim=2))
    if batch == 1:
        return frame_rgb.view(ry, rx, 3), frame_hit.view(ry, rx)
    return frame_rgb, frame_hit


_GATHER_MODE = {"mode": "gather"}


def gather_frame(local_buf, res, rank, world, stripe_h, dst=0, gathered=None, async_op=False):
    """One collective for a frame (or a batch of frames, rendered back to back into one buffer): every
    rank's packed stripe buffer to rank `dst` (RCCL on GPUs, gloo in the CPU tests).  Returns (work handle or None, gather list or None).
    `gather` is the natural all-to-one; should a backend build not provide it, the first failure
    switches this process group to `all_gather` (same bytes into rank `dst`, the other ranks simply
    ignore what they receive) - every rank hits the same error at the same call, so they switch
    together."""
    import torch
    import torch.distributed as dist
    if _GATHER_MODE["mode"] == "gather":
        if rank == dst and gathered is None:
            gathered = [torch.empty_like(local_buf) for _ in range(world)]
        try:
            work = dist.gather(local_buf, gathered if rank == dst else None, dst=dst, async_op=async_op)
            return work, gathered
        except (RuntimeError, NotImplementedError):
            _GATHER_MODE["mode"] = "all_gather"
    if gathered is None:
        gathered = [torch.empty_like(local_buf) for _ in range(world)]
    work = dist.all_gather(gathered, local_buf, async_op=async_op)
    return work, gathered


def assemble_frame8(gathered, res, world, stripe_h, frame8=None, batch=1):
    """Same de-interleave for u8 frames (img_Data, 3 B/pixel): the payload bench.py gathers by default."""
    import torch
    rx, ry = res
    n_str = ry // (stripe_h * world)
    if frame8 is None:
        frame8 = torch.empty((batch, ry, rx, 3), dtype=torch.uint8, device=gathered[0].device)
    parts = [g.view(batch, n_str, stripe_h, rx, 3) for g in gathered]
    frame8.view(batch, n_str, world, stripe_h, rx, 3).copy_(torch.stack(parts, dim=2))
    return frame8.view(ry, rx, 3) if batch == 1 else frame8
