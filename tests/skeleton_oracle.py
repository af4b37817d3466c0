"""NumPy restatement of the skeleton stage (tests only): the thinning table of Zhang & Suen, CACM 27(3), 1984, the
two-sub-iteration thinning loop with its iteration count, and the node detection with its list order.

Written as the definition reads -- a zero-padded array and eight shifted views of it -- and independently of the kernel's
bit-packed words (csrc/skeleton.hip).  Conventions: a pixel is on when its byte is non-zero, pixels outside the image are off,
N is the smaller index on axis 0 and W the smaller index on axis 1.  An on pixel's neighbour code is
NW 1 + N 2 + NE 4 + E 8 + SE 16 + S 32 + SW 64 + W 128.
"""
import numpy as np

# (axis-0 step, axis-1 step, weight in the code) of the eight neighbours
NEIGHBOURS = {"NW": (-1, -1, 1), "N": (-1, 0, 2), "NE": (-1, 1, 4), "E": (0, 1, 8), "SE": (1, 1, 16), "S": (1, 0, 32),
              "SW": (1, -1, 64), "W": (0, -1, 128)}
WALK = ["N", "NE", "E", "SE", "S", "SW", "W", "NW"]   # A counts off -> on steps along this walk, closed back on N


def zhang_suen_table():
    """uint8 [256]: bit 0 = delete in the first sub-iteration, bit 1 = delete in the second."""
    table = np.zeros(256, np.uint8)
    for code in range(256):
        on = {name: (code // wt) % 2 for name, (_, _, wt) in NEIGHBOURS.items()}
        b = sum(on.values())
        ring = [on[name] for name in WALK]
        a = sum(1 for i in range(8) if ring[i] == 0 and ring[(i + 1) % 8] == 1)
        if not (2 <= b <= 6 and a == 1):
            continue
        if on["N"] * on["E"] * on["S"] == 0 and on["E"] * on["S"] * on["W"] == 0:
            table[code] |= 1
        if on["N"] * on["E"] * on["W"] == 0 and on["N"] * on["S"] * on["W"] == 0:
            table[code] |= 2
    return table


def _shifted(img01):
    """name -> the [H, W] array of that neighbour's value (0 / 1), off outside the image."""
    h, w = img01.shape
    padded = np.zeros((h + 2, w + 2), np.uint8)
    padded[1:-1, 1:-1] = img01
    return {name: padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for name, (dy, dx, _) in NEIGHBOURS.items()}


def neighbour_codes(img01):
    views = _shifted(img01)
    code = np.zeros(img01.shape, np.int64)
    for name, (_, _, wt) in NEIGHBOURS.items():
        code += wt * views[name].astype(np.int64)
    return code


def thin(mask, table=None, max_iters=None):
    """(skeleton uint8 [H, W] of 0 / 1, iterations run including the last idle one; -1 = not converged after max_iters)."""
    table = zhang_suen_table() if table is None else np.asarray(table, np.uint8)
    img = (np.asarray(mask) != 0).astype(np.uint8)
    it = 0
    while True:
        it += 1
        deleted = False
        for bit in (1, 2):
            kill = (img == 1) & ((table[neighbour_codes(img)] & bit) != 0)
            if kill.any():
                deleted = True
                img = np.where(kill, 0, img).astype(np.uint8)
        if not deleted:
            return img, it
        if max_iters is not None and it >= max_iters:
            return img, -1


def crossings(img):
    """A(p) for every pixel (also the off ones): off -> on steps along WALK, closed."""
    views = _shifted((np.asarray(img) != 0).astype(np.uint8))
    a = np.zeros(np.asarray(img).shape, np.int64)
    for i, name in enumerate(WALK):
        a += ((views[name] == 0) & (views[WALK[(i + 1) % 8]] == 1)).astype(np.int64)
    return a


def node_class(img):
    """uint8 [H, W]: 0 = not a node, else A(p) (1 = end point, >= 3 = branching point)."""
    a = crossings(img)
    is_node = (np.asarray(img) != 0) & ((a == 1) | (a >= 3))
    return np.where(is_node, a, 0).astype(np.uint8)


def nodes(img):
    """int32 [K, 2]: (axis-0 index, axis-1 index) of the nodes in row-major order of `img` as given."""
    return np.argwhere(node_class(img) != 0).astype(np.int32).reshape(-1, 2)
