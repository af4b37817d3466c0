"""NumPy restatement of the connected-component stage (csrc/ccl.hip) -- no scipy, so it runs wherever the suite runs;
tests/test_ccl_cpu.py pins it to scipy.ndimage where scipy is installed.

  erode2x2            binary_erosion(np.pad(a, 1), np.ones((2, 2)))[1:-1, 1:-1]: (i, j) stays on iff (i-1..i) x (j-1..j) are on
  label               scipy.ndimage.label: components numbered in row-major order of their first pixel; connectivity 1 = 4
                      neighbours, 2 = 8.  Runs of on pixels per row, union-find over runs that touch in adjacent rows (the
                      smaller run number is always the root), roots ranked in run order -- run order is first-pixel order.
  stats               per label: area, half-open bounding box (find_objects), int64 sums of r, c, r*r, c*c, r*c
  centers             (sum_r // area, sum_c // area) = int() of center_of_mass
  dense_nodes         find_dense_skeleton_nodes of the reference's extract_network.py, on the array as given
  merge_nodes         its add_dense_nodes: a dense node is kept iff no ORIGINAL node is at squared distance < min_d2
"""
import numpy as np


def erode2x2(a):
    on = np.asarray(a) != 0
    out = np.zeros(on.shape, bool)
    out[1:, 1:] = on[1:, 1:] & on[:-1, 1:] & on[1:, :-1] & on[:-1, :-1]
    return out


def _runs(on):
    """Runs of on pixels in row-major order: (row, start, end) arrays, end exclusive."""
    h, w = on.shape
    padded = np.zeros((h, w + 2), np.int8)
    padded[:, 1:-1] = on
    d = np.diff(padded, axis=1)
    rows, starts = np.nonzero(d == 1)
    _, ends = np.nonzero(d == -1)
    return rows, starts, ends


def label(a, connectivity=1):
    """-> (labels int32 [h, w], K)"""
    assert connectivity in (1, 2)
    on = np.asarray(a) != 0
    rows, starts, ends = _runs(on)
    nrun = len(rows)
    parent = list(range(nrun))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    reach = connectivity - 1            # 8 neighbours: runs that only touch diagonally are joined too
    first = np.searchsorted(rows, np.arange(on.shape[0] + 1))      # first run of every row
    S, E = starts.tolist(), ends.tolist()
    for y in range(1, on.shape[0]):
        i, iend, j, jend = first[y - 1], first[y], first[y], first[y + 1]
        while i < iend and j < jend:
            if S[i] < E[j] + reach and S[j] < E[i] + reach:
                ra, rb = find(i), find(j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if E[i] < E[j]:
                i += 1
            else:
                j += 1
    roots = np.array([find(x) for x in range(nrun)], np.int64)
    is_root = roots == np.arange(nrun)
    number = np.cumsum(is_root)          # roots in run order = components in order of their first pixel
    run_label = number[roots] if nrun else np.zeros(0, np.int64)
    out = np.zeros(on.shape, np.int32)
    flat = out.reshape(-1)
    w = on.shape[1]
    lengths = ends - starts
    if nrun:
        offs = np.repeat(rows * w + starts - np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths) + np.arange(lengths.sum())
        flat[offs] = np.repeat(run_label, lengths)
    return out, int(is_root.sum())


def stats(labels, k=None):
    """-> dict(area int32 [K], bbox int32 [K, 4] = r0, c0, r1, c1, sums int64 [K, 5] = r, c, rr, cc, rc)"""
    labels = np.asarray(labels)
    k = int(labels.max(initial=0)) if k is None else k
    r, c = np.nonzero(labels)
    lab = labels[r, c].astype(np.int64)
    order = np.argsort(lab, kind="stable")
    r, c, lab = r[order].astype(np.int64), c[order].astype(np.int64), lab[order]
    cut = np.searchsorted(lab, np.arange(1, k + 2))
    assert (np.diff(cut) > 0).all(), "a label without pixels"
    at = cut[:-1]
    red = lambda f, v: f.reduceat(v, at) if k else np.zeros(0, np.int64)  # noqa: E731
    return {"area": np.diff(cut).astype(np.int32),
            "bbox": np.stack([red(np.minimum, r), red(np.minimum, c), red(np.maximum, r) + 1, red(np.maximum, c) + 1],
                             axis=1).astype(np.int32).reshape(k, 4),
            "sums": np.stack([red(np.add, v) for v in (r, c, r * r, c * c, r * c)], axis=1).astype(np.int64).reshape(k, 5)}


def pack(s):
    """The statistics as rows of the C struct dsg_cc_stat, viewed as int64 [K, 8]."""
    k = len(s["area"])
    words = np.zeros((k, 16), np.int32)
    words[:, 0] = s["area"]
    words[:, 1:5] = s["bbox"]
    raw = words.view(np.int64).reshape(k, 8).copy()
    raw[:, 3:8] = s["sums"]
    return raw


def centers(s):
    area = s["area"].astype(np.int64)
    return np.stack([s["sums"][:, 0] // area, s["sums"][:, 1] // area], axis=1).astype(np.int32).reshape(-1, 2)


def dense_nodes(skel):
    lab, k = label(erode2x2(skel), 1)
    return centers(stats(lab, k))


def merge_nodes(nodes, dense, min_d2=25):
    """[*nodes, *kept]: a dense node is dropped iff an original node is at squared distance < min_d2."""
    whole = all(np.issubdtype(np.asarray(x).dtype, np.integer) or np.asarray(x).size == 0 for x in (nodes, dense))
    kind = np.int64 if whole else np.float64     # (the engine's coordinates are integers; the rule itself is not tied to them)
    nodes = np.asarray(nodes, kind).reshape(-1, 2)
    dense = np.asarray(dense, kind).reshape(-1, 2)
    keep = [d for d in dense if not (((nodes - d) ** 2).sum(1) < min_d2).any()]
    out = np.concatenate([nodes, np.array(keep, kind).reshape(-1, 2)])
    return out.astype(np.int32) if whole else out
