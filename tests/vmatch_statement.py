"""The sequential matcher of tests/matcher_statement.py restated over a GIVEN distance matrix: okvis::DenseMatcher::match with ONE
matcher thread for an algorithm whose distance(a, b) is dist[a][b] — for the verified matcher (okvis_fe_match_verified) the Hamming
distance where it is under the threshold and verifyMatch(a, b) holds, FLT_MAX elsewhere.  It imports nothing from the product.

    listBIteration  okvis_matcher/include/okvis/implementation/DenseMatcher.hpp:153-179
    the row loop    ... :183-225 (doWorkLinearMatching)
    assignbest      okvis_matcher/src/DenseMatcher.cpp:69-111
    the final loop  ... DenseMatcher.hpp:92-122 (matchBody)
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def _mask(m, n):
    return np.zeros(n, bool) if m is None else np.asarray(m).astype(bool)


def distance_matrix(hamming, threshold, verified=None):
    """[n_a][n_b] float32: the Hamming distance where it is < threshold (and verified), FLT_MAX elsewhere"""
    ham = np.asarray(hamming).astype(np.float32)
    keep = ham < np.float32(threshold)
    if verified is not None:
        keep &= np.asarray(verified).astype(bool)
    return np.where(keep, ham, FLT_MAX).astype(np.float32)


def match(dist, threshold, num_best=4, use_ratio=False, ratio_threshold=0.0, skip_a=None, skip_b=None):
    """dist [n_a][n_b] float32 -> pair_a [n_b] int32, pair_dist [n_b] float32, calls: the (a, b, distance) of every setBestMatch in
    order, lists: {a: [(b, distance)] * num_best} as listBIteration left them"""
    dist = np.asarray(dist, np.float32)
    n_a, n_b = dist.shape
    threshold = np.float32(threshold)
    skip_a, skip_b = _mask(skip_a, n_a), _mask(skip_b, n_b)
    initial = FLT_MAX if use_ratio else threshold
    pair_a = np.full(n_b, -1, np.int32)
    pair_dist = np.full(n_b, FLT_MAX, np.float32)
    best = {}

    def assignbest(a, start):
        # the reference recurses as its last act (assignbest(old, ..., 1); return): the same chain as a loop
        while a is not None:
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
            a, start = displaced, 1

    for a in range(n_a):
        if skip_a[a]:
            continue
        lst = [(-1, initial)] * num_best
        # b in ascending order; a distance of FLT_MAX is never below a list's last entry (at most FLT_MAX), so only the others are
        # visited
        for b in np.flatnonzero((dist[a] < FLT_MAX) & ~skip_b):
            d = dist[a, b]
            if d < lst[-1][1]:
                pos = 0                               # std::lower_bound on the distance: in front of equal entries
                while lst[pos][1] < d:
                    pos += 1
                lst = lst[:pos] + [(int(b), d)] + lst[pos:-1]
        best[a] = lst
        assignbest(a, 0)

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
    return pair_a, pair_dist, calls, best


def accepted_mask(calls, n_b):
    m = np.zeros(n_b, bool)
    for _, b, _ in calls:
        m[b] = True
    return m


def scene_statistics(dist_verified, dist_plain, threshold, num_best, skip_a=None, skip_b=None):
    """what a scene exercises, as fractions of its rows of A: rows with two or more verified entries in their list, rows whose list
    holds a tie, rows that do not keep their first choice, rows whose list differs from the unverified matcher's"""
    pair_a, _, _, lists = match(dist_verified, threshold, num_best, False, 0.0, skip_a, skip_b)
    _, _, _, plain = match(dist_plain, threshold, num_best, False, 0.0, skip_a, skip_b)
    n = max(1, dist_verified.shape[0])
    two = tie = lost = changed = 0
    for a, lst in lists.items():
        kept = [d for b, d in lst if b != -1]
        two += len(kept) >= 2
        tie += len(set(kept)) < len(kept)
        lost += lst[0][0] != -1 and pair_a[lst[0][0]] != a
        changed += [b for b, _ in lst] != [b for b, _ in plain[a]]
    return {"two_or_more": two / n, "tie": tie / n, "lost_first": lost / n, "changed": changed / n}
