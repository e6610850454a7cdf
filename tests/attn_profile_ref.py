"""fp64 restatement of g3_attn_pattern_profile_bf16 / g3_attn_pattern_select (include/gen3c_hip.h), from the RANGE TABLE - not from the bitmask the
kernel reads: for sample row r of block r // 256, batch b, head h

    l_j = softmax_scale * (q_r . k_j) over all S keys,  m = max_j l_j,
    recall[b][h][i][p] = sum over the keys j of the list (pattern p, block of sample_rows[i]) of exp(l_j - m) / sum over all j of exp(l_j - m),
    score[h][p] = mean of recall over b and i,  head_pattern[h] = argmax_p score[h][p] with the lowest index on ties.

Inputs are the bf16 tensors the kernel sees (their values are exact in fp64)."""
import math

import numpy as np

Q_ROWS = 256


def key_mask(ranges, S: int, pattern: int, block: int) -> np.ndarray:
    """bool [S]: the keys of the list (pattern, block); the list ends at the first n_keys == 0."""
    mask = np.zeros(S, dtype=bool)
    for first, n in np.asarray(ranges)[pattern, block].tolist():
        if n == 0:
            break
        mask[first:first + n] = True
    return mask


def recall_ref(q, k, S: int, B: int, H: int, ranges, sample_rows, softmax_scale=None, flip=None) -> np.ndarray:
    """q, k: torch [S*B, H*128] (row s*B + b; any strides) -> float64 [B, H, n, n_patterns]. flip = (i, pattern, tile): that sample row's membership of
    that 64-key tile inverted (the tests' teeth)."""
    ranges = np.asarray(ranges)
    scale = 1.0 / math.sqrt(128) if softmax_scale is None else float(softmax_scale)
    rows = [int(r) for r in sample_rows]
    n_pat = ranges.shape[0]
    out = np.zeros((B, H, len(rows), n_pat), dtype=np.float64)
    qd = q.detach().cpu().double().numpy().reshape(S, B, H, 128)
    kd = k.detach().cpu().double().numpy().reshape(S, B, H, 128)
    masks = {}
    for i, r in enumerate(rows):
        for p in range(n_pat):
            mk = key_mask(ranges, S, p, r // Q_ROWS)
            if flip is not None and flip[0] == i and flip[1] == p:
                mk = mk.copy()
                mk[flip[2] * 64:(flip[2] + 1) * 64] ^= True
            masks[i, p] = mk
    for b in range(B):
        for h in range(H):
            logits = scale * (qd[rows, b, h] @ kd[:, b, h].T)  # [n, S]
            w = np.exp(logits - logits.max(axis=1, keepdims=True))
            den = w.sum(axis=1)
            for i in range(len(rows)):
                for p in range(n_pat):
                    out[b, h, i, p] = w[i, masks[i, p]].sum() / den[i]
    return out


def select_ref(recall: np.ndarray):
    """float64 recall [B, H, n, n_patterns] -> (score [H, n_patterns], head_pattern [H] - the first maximum)."""
    score = recall.mean(axis=(0, 2))
    return score, np.argmax(score, axis=1).astype(np.int32)


def hand_table_832() -> np.ndarray:
    """S = 832 (blocks of 256, 256, 256 and 64 rows), three hand-made patterns: the block's own rows; a sink of two tiles plus the last two tiles; three
    stripes that move with the block."""
    S, tab = 832, np.zeros((3, 4, 3, 2), dtype=np.int32)
    for b in range(4):
        tab[0, b, 0] = (256 * b, min(256, S - 256 * b))
        tab[1, b, :2] = [(0, 128), (704, 128)]
        tab[2, b] = [(64 * b, 64), (64 * b + 192, 128), (640, 192)]
    return tab


SAMPLE_ROWS_832 = [0, 100, 255, 256, 300, 511, 512, 600, 767, 768, 800, 830, 831]
