"""A plain, sequential restatement of okvis::DenseMatcher::match with ONE matcher thread, for an algorithm whose distance(a, b) is
the Hamming distance of two binary descriptors where that is below the threshold and FLT_MAX elsewhere — the referee of
okvis_fe_hamming_candidates / okvis_fe_match_descriptors.  It imports nothing from the product; tests/golden/dense_matcher.npz
(recorded from the reference's own DenseMatcher.cpp) pins it.

    listBIteration  okvis_matcher/include/okvis/implementation/DenseMatcher.hpp:153-179
    the row loop    ... :183-225 (doWorkLinearMatching)
    assignbest      okvis_matcher/src/DenseMatcher.cpp:69-111
    the final loop  ... DenseMatcher.hpp:92-122 (matchBody)
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def hamming_matrix(desc_a, desc_b):
    """[n_a][n_b] int: bits that differ"""
    a = np.unpackbits(np.ascontiguousarray(desc_a, np.uint8), axis=1).astype(np.float32)
    b = np.unpackbits(np.ascontiguousarray(desc_b, np.uint8), axis=1).astype(np.float32)
    # bits of the XOR = ones(a) + ones(b) - 2 common ones; at most 512, so float32 holds every term exactly
    return (a.sum(1)[:, None] + b.sum(1)[None, :] - 2 * (a @ b.T)).astype(np.int32)


def _mask(m, n):
    return np.zeros(n, bool) if m is None else np.asarray(m).astype(bool)


def candidates(desc_a, desc_b, threshold, skip_a=None, skip_b=None):
    """-> pairs [n][2] int32 in ascending (a, b) order, dist [n] float32: keypoints in play, (float)distance < threshold"""
    d = hamming_matrix(desc_a, desc_b).astype(np.float32)
    keep = d < np.float32(threshold)
    keep &= ~_mask(skip_a, len(desc_a))[:, None]
    keep &= ~_mask(skip_b, len(desc_b))[None, :]
    a, b = np.nonzero(keep)            # row-major: ascending (a, b)
    return np.stack([a, b], 1).astype(np.int32).reshape(-1, 2), d[a, b]


def match(desc_a, desc_b, threshold, num_best=4, use_ratio=False, ratio_threshold=0.0, skip_a=None, skip_b=None, events=None):
    """-> pair_a [n_b] int32, pair_dist [n_b] float32, calls: the (a, b, distance) of every setBestMatch, in order.
    `events` (a dict) receives what the tie rules met: rows_with_equal_kept, equal_to_last_turned_away, max_chain_depth."""
    n_a, n_b = len(desc_a), len(desc_b)
    threshold = np.float32(threshold)
    skip_a, skip_b = _mask(skip_a, n_a), _mask(skip_b, n_b)
    ham = hamming_matrix(desc_a, desc_b).astype(np.float32) if n_a and n_b else np.zeros((n_a, n_b), np.float32)
    dist = np.where(ham < threshold, ham, FLT_MAX).astype(np.float32)
    initial = FLT_MAX if use_ratio else threshold
    pair_a = np.full(n_b, -1, np.int32)
    pair_dist = np.full(n_b, FLT_MAX, np.float32)
    best = {}
    ev = {"rows_with_equal_kept": 0, "equal_to_last_turned_away": 0, "max_chain_depth": 0}

    def assignbest(a, start, depth):
        # the reference recurses as its last act (assignbest(old, ..., 1); return): the same chain as a loop
        while a is not None:
            ev["max_chain_depth"] = max(ev["max_chain_depth"], depth)
            lst, k, displaced = best[a], start, None
            while k < num_best and lst[k][0] != -1:
                b, d = lst[k]
                if pair_a[b] == -1:
                    pair_a[b], pair_dist[b] = a, d
                    return
                if d < pair_dist[b]:
                    displaced = int(pair_a[b])
                    pair_a[b], pair_dist[b] = a, d
                    break
                k += 1
            a, start, depth = displaced, 1, depth + 1

    for a in range(n_a):
        if skip_a[a]:
            continue
        lst = [(-1, initial)] * num_best
        turned = 0
        for b in range(n_b):
            if skip_b[b]:
                continue
            d = dist[a, b]
            if d < lst[-1][1]:
                pos = 0                               # std::lower_bound on the distance: in front of equal entries
                while lst[pos][1] < d:
                    pos += 1
                lst = lst[:pos] + [(b, d)] + lst[pos:-1]
            elif d == lst[-1][1] and lst[-1][0] != -1:
                turned += 1
        best[a] = lst
        kept = [d for i, d in lst if i != -1]
        ev["rows_with_equal_kept"] += len(set(kept)) < len(kept)
        ev["equal_to_last_turned_away"] += turned
        assignbest(a, 0, 0)

    calls = []
    for b in range(n_b):
        if not pair_dist[b] < threshold:
            continue
        a = int(pair_a[b])
        if use_ratio:
            lst = best[a]
            if lst[1][0] != -1:
                first, second = lst[0][1], lst[1][1]
                with np.errstate(divide="ignore", over="ignore"):
                    if first == 0 or np.float32(second) / np.float32(first) > np.float32(ratio_threshold):
                        calls.append((a, b, float(pair_dist[b])))
            else:
                calls.append((a, b, float(pair_dist[b])))
        else:
            calls.append((a, b, float(pair_dist[b])))
    if events is not None:
        events.update(ev)
    return pair_a, pair_dist, calls


def accepted_mask(calls, n_b):
    m = np.zeros(n_b, bool)
    for _, b, _ in calls:
        m[b] = True
    return m
