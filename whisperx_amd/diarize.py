"""Speaker assignment: the drop-in for the reference's assign_word_speakers
(whisperx/diarize.py:35-67), the step transcribe.py:222 runs between align() and the writers.

It needs only a table of (start, end, speaker) turns, from any diarizer; the reference's
DiarizationPipeline (pyannote's pipeline and its gated models) is not part of this package.

Semantics ("Speaker assignment"): the queries are every segment and every word of
it that has a 'start' key.  For a query (qs, qe) and every turn, x = min(end, qe) -
max(start, qs) in fp64.  fill_nearest=False: the turns with x > 0 take part, and a query no
turn takes part in is left alone (an existing 'speaker' key stays).  fill_nearest=True: every
turn takes part, negative x included; a NaN x adds nothing but its speaker still has a sum.
Each speaker's sum runs over its participating turns in table row order with Kahan
compensation (what pandas' groupby().sum() does; a plain sum picks another speaker on some
inputs).  The largest sum wins, the first label in sorted label order among equal sums.

Limits: times are taken as float64; speaker labels are non-null (and sortable); non-finite
turn times follow plain IEEE arithmetic in the Kahan recurrence (pandas resets a NaN
compensation term; that is not reproduced).

All queries of a call — or of a whole corpus, assign_word_speakers_batch — go to the GPU in
one launch of wx_assign_speakers.  A host route with the same semantics in numpy (the same
group and row order, the same recurrence) runs with device='cpu' or where no HIP device or
library is present.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np

from .vad import Segment  # noqa: F401  (diarize.Segment of the reference)


def _kernel_available() -> bool:
    import torch

    from . import _lib

    return torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH)


def _queries(transcript_result):
    """The reference's evaluation order: each segment, then its words that have 'start'.
    Returns (targets, q_start, q_end): the dicts to label and their times."""
    targets, qs, qe = [], [], []
    for seg in transcript_result["segments"]:
        targets.append(seg)
        qs.append(seg["start"])
        qe.append(seg["end"])
        if "words" in seg:
            for word in seg["words"]:
                if "start" in word:
                    targets.append(word)
                    qs.append(word["start"])
                    qe.append(word["end"])
    return targets, np.asarray(qs, dtype=np.float64).reshape(-1), np.asarray(qe, dtype=np.float64).reshape(-1)


def assign_speakers_host(turns, q_start, q_end, q_off, fill_nearest: bool = False):
    """wx_assign_speakers on the host (numpy, vectorised over a file's queries; one step per
    turn, in the packed group and row order, with the kernel's Kahan recurrence).  Returns
    (speaker [Q] int32, best_sum [Q] float64) like _lib.assign_speakers."""
    q_start = np.asarray(q_start, dtype=np.float64)
    q_end = np.asarray(q_end, dtype=np.float64)
    Q = q_start.size
    speaker = np.full(Q, -1, dtype=np.int32)
    best_sum = np.zeros(Q, dtype=np.float64)
    fill = bool(fill_nearest)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(turns.F):
            a, b = int(q_off[f]), int(q_off[f + 1])
            if b <= a:
                continue
            qs, qe = q_start[a:b], q_end[a:b]
            n = b - a
            have = np.zeros(n, dtype=bool)
            best = np.zeros(n)
            rank = np.full(n, -1, dtype=np.int32)
            g0, g1 = int(turns.grp_off[f]), int(turns.grp_off[f + 1])
            for g in range(g0, g1):
                t0, t1 = int(turns.turn_off[g]), int(turns.turn_off[g + 1])
                s = np.zeros(n)
                c = np.zeros(n)
                exists = np.full(n, fill and t1 > t0)
                for t in range(t0, t1):
                    x = np.minimum(turns.end[t], qe) - np.maximum(turns.start[t], qs)
                    part = ~np.isnan(x) if fill else x > 0
                    if not part.any():
                        continue
                    y = x - c
                    tt = s + y
                    c = np.where(part, (tt - s) - y, c)
                    s = np.where(part, tt, s)
                    exists |= part
                take = exists & (~have | (s > best) | (np.isnan(best) & ~np.isnan(s)))
                best = np.where(take, s, best)
                rank[take] = g - g0
                have |= take
            speaker[a:b] = rank
            best_sum[a:b] = np.where(have, best, 0.0)
    return speaker, best_sum


def assign_queries(tables, q_start, q_end, q_off, fill_nearest: bool = False, device=None):
    """The assignment itself, on the route `device` selects: tables = [(start, end, speaker
    labels)] per file, queries of file f = q_off[f] .. q_off[f + 1] of q_start / q_end.  Returns
    (speaker [Q] int32: index into the file's labels, or -1; best_sum [Q] float64: the winning
    Kahan sum, 0.0 with -1; labels: per file, its labels in sorted order)."""
    from . import _lib

    turns = _lib.SpeakerTurns(tables)
    q_start = np.asarray(q_start, dtype=np.float64).reshape(-1)
    q_end = np.asarray(q_end, dtype=np.float64).reshape(-1)
    if device is None:
        on_host = not _kernel_available()
    else:
        import torch

        on_host = torch.device(device).type != "cuda"  # a HIP device without a library or GPU raises below
    if on_host or q_start.size == 0:
        speaker, best = assign_speakers_host(turns, q_start, q_end, q_off, fill_nearest)
    else:
        spk_d, best_d = _lib.assign_speakers(turns, q_start, q_end, q_off, fill_nearest, device=device)
        speaker, best = spk_d.cpu().numpy(), best_d.cpu().numpy()
    return speaker, best, turns.labels


def assign_word_speakers_batch(pairs: Sequence[Tuple[object, dict]], fill_nearest: bool = False,
                               device=None) -> List[dict]:
    """assign_word_speakers over a corpus: `pairs` is a list of (diarize_df, transcript_result),
    all of whose queries are assigned in one launch.  Each pair is mutated exactly as the single
    call mutates it; returns the transcript results.  Every file's queries are gathered before
    anything is assigned, so a malformed transcript (a word with 'start' and no 'end') raises
    with no pair mutated, where the reference run file by file would have labelled the earlier
    files."""
    pairs = list(pairs)
    tables, all_targets, qs_l, qe_l, q_off = [], [], [], [], [0]
    for df, result in pairs:
        tables.append((df["start"], df["end"], np.asarray(df["speaker"]).tolist()))
        targets, qs, qe = _queries(result)
        all_targets.append(targets)
        qs_l.append(qs)
        qe_l.append(qe)
        q_off.append(q_off[-1] + len(targets))
    q_start = np.concatenate(qs_l) if qs_l else np.zeros(0)
    q_end = np.concatenate(qe_l) if qe_l else np.zeros(0)
    speaker, _, labels = assign_queries(tables, q_start, q_end, np.asarray(q_off, dtype=np.int64), fill_nearest,
                                        device)
    for f, ((df, _), targets) in enumerate(zip(pairs, all_targets)):
        a = q_off[f]
        for k, target in enumerate(targets):
            r = int(speaker[a + k])
            if r >= 0:
                target["speaker"] = labels[f][r]
        if targets:
            # the two columns the reference leaves behind: those of the last query evaluated
            last_s, last_e = q_start[a + len(targets) - 1], q_end[a + len(targets) - 1]
            with np.errstate(invalid="ignore"):
                df["intersection"] = np.minimum(df["end"], last_e) - np.maximum(df["start"], last_s)
                df["union"] = np.maximum(df["end"], last_e) - np.minimum(df["start"], last_s)
    return [result for _, result in pairs]


def assign_word_speakers(diarize_df, transcript_result, fill_nearest: bool = False, device=None):
    """The reference's assign_word_speakers(diarize_df, transcript_result, fill_nearest).

    diarize_df: anything with ["start"], ["end"], ["speaker"] item access and item assignment
    (a pandas DataFrame, or a plain dict of arrays).  transcript_result is mutated (segments
    and timed words gain 'speaker') and returned; diarize_df gains the reference's
    'intersection' and 'union' columns, holding the last query's values (none when there are
    no segments).  device: None = the HIP kernel when a device is available, else the host
    route; 'cpu' = the host route; a HIP device ('cuda', 'cuda:0', a torch.device) = the kernel
    (an error when there is none).
    Stated limits: see the module docstring."""
    assign_word_speakers_batch([(diarize_df, transcript_result)], fill_nearest=fill_nearest, device=device)
    return transcript_result
