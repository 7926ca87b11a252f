"""Packing of a list of clips into network passes (Videoseal.embed_clips / detect_clips / extract_messages).  Pure Python on plain data:
lengths in, lists of ints and tuples out -- no torch, no GPU.

Span   at most chunk_size * step_size consecutive frames of ONE clip, starting at a multiple of that inside the clip: exactly the piece
       `embed(clip, is_video=True)` runs as one chunk (videoseal.py:291-297).  Its key frames are its frames 0, step, 2 step, ...; the watermark
       expansion ('repeat', 'alternate', 'interpolate') never looks outside its span, as in the per-clip call.
Embed pass   a run of consecutive spans in list order, clip after clip, closed before the span that would take it past KEY_BATCH key frames
       (the batch at which the U-Net's dominant kernel has a tile per CU, streaming.py); a pass always holds at least one span.
Detect pass  a run of at most DET_BATCH consecutive frames of the flattened list, cut anywhere: the extractor is per frame.

A slot is (clip, start, frames, first_frame, first_key): frames [start, start + frames) of clip `clip` are frames first_frame ... of the pass,
their key frames are key frames first_key ... of the pass (vs_clip_desc_t).  Detect slots carry no first_key."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from .streaming import DET_BATCH, KEY_BATCH

Slot = Tuple[int, int, int, int, int]


def spans(lengths: Sequence[int], step: int, chunk_size: int) -> List[Tuple[int, int, int]]:
    """(clip, start, frames) of every span, in list order; a clip without frames has none"""
    if step < 1 or chunk_size < 1:
        raise ValueError(f"step ({step}) and chunk_size ({chunk_size}) must be at least 1")
    per = chunk_size * step
    return [(c, a, min(per, int(n) - a)) for c, n in enumerate(lengths) for a in range(0, int(n), per)]


def embed_passes(lengths: Sequence[int], step: int, chunk_size: int, key_batch: int = KEY_BATCH) -> List[Tuple[List[Slot], List[int]]]:
    """-> [(slots, rows)]: the slots of every embed pass and, per key frame of the pass, the clip whose message row it takes"""
    passes: List[Tuple[List[Slot], List[int]]] = []
    slots: List[Slot] = []
    rows: List[int] = []
    frames = 0
    for c, a, n in spans(lengths, step, chunk_size):
        keys = (n + step - 1) // step
        if slots and len(rows) + keys > key_batch:
            passes.append((slots, rows))
            slots, rows, frames = [], [], 0
        slots.append((c, a, n, frames, len(rows)))
        rows.extend([c] * keys)
        frames += n
    if slots:
        passes.append((slots, rows))
    return passes


def detect_passes(lengths: Sequence[int], det_batch: int = DET_BATCH) -> List[List[Tuple[int, int, int, int]]]:
    """-> per detect pass its slots (clip, start, frames, first_frame): the flattened list in runs of at most det_batch frames"""
    if det_batch < 1:
        raise ValueError(f"det_batch ({det_batch}) must be at least 1")
    passes: List[List[Tuple[int, int, int, int]]] = []
    cur: List[Tuple[int, int, int, int]] = []
    used = 0
    for c, n in enumerate(lengths):
        a = 0
        while a < int(n):
            take = min(int(n) - a, det_batch - used)
            cur.append((c, a, take, used))
            a, used = a + take, used + take
            if used == det_batch:
                passes.append(cur)
                cur, used = [], 0
    if cur:
        passes.append(cur)
    return passes


def first_rows(lengths: Sequence[int]) -> List[int]:
    """prefix sums of the lengths: clip i owns rows [first_rows[i], first_rows[i + 1]) of the flattened list"""
    out = [0]
    for n in lengths:
        out.append(out[-1] + int(n))
    return out
