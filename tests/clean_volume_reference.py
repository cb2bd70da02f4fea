"""clean_volume (reference utils/tools.py:34-50) restated in plain numpy, in this project's words: label the set voxels' connected components,
keep the largest.  skimage is not needed: the labelling is a flood fill with an explicit stack.

  * a voxel is set if its value is > 0; neighbours are the 26 (connectivity 3) or 6 (connectivity 1) voxels around it, inside the volume only;
  * components are numbered 1, 2, ... in the C order of their first voxels -- skimage.measure.label's and scipy.ndimage.label's numbering
    (tests/test_clean_volume_cpu.py checks the latter);
  * regionprops lists the regions in label order and np.argmax takes the first maximum: the largest component wins, a tie goes to the one
    whose first voxel comes first;
  * the reference returns `label` with every other region zeroed: the winner's voxels hold ITS LABEL NUMBER, not 1; an empty volume
    (num < 1) is returned as it came."""
import numpy as np


def _offsets(connectivity):
    if connectivity not in (1, 3):
        raise ValueError("connectivity 1 or 3")
    r = (-1, 0, 1)
    offs = [(a, b, c) for a in r for b in r for c in r if (a, b, c) != (0, 0, 0)]
    if connectivity == 1:
        offs = [o for o in offs if abs(o[0]) + abs(o[1]) + abs(o[2]) == 1]
    return offs


def label(mask, connectivity=3):
    """mask (nx, ny, nz), set where > 0 -> (labels int64 of the same shape, 0 = background, components numbered from 1 in the C order of
    their first voxels; number of components).  The fill runs on a copy padded by one clear voxel per side, flat, so that a neighbour is an
    index offset and needs no bounds test."""
    m = np.asarray(mask) > 0
    nx, ny, nz = m.shape
    sy, sx = nz + 2, (ny + 2) * (nz + 2)
    todo = bytearray(np.pad(m, 1).astype(np.uint8).tobytes())        # 1 = set and not labelled yet
    lab = [0] * len(todo)
    offs = [a * sx + b * sy + c for a, b, c in _offsets(connectivity)]
    num = 0
    for start in np.flatnonzero(np.pad(m, 1).reshape(-1)).tolist():   # C order: the first unlabelled set voxel opens the next label
        if not todo[start]:
            continue
        num += 1
        todo[start] = 0
        lab[start] = num
        stack = [start]
        while stack:
            p = stack.pop()
            for o in offs:
                q = p + o
                if todo[q]:
                    todo[q] = 0
                    lab[q] = num
                    stack.append(q)
    lab = np.array(lab, dtype=np.int64).reshape(nx + 2, ny + 2, nz + 2)[1:-1, 1:-1, 1:-1]
    return np.ascontiguousarray(lab), num


def clean_volume(mask, connectivity=3):
    """-> (result, (N, size, first index, label number)): the reference's return value (the input itself when N < 1, else the int64 label
    volume with every region but the largest zeroed), the number of components, the winner's size, the linear C-order index of its first
    voxel (-1 when empty) and its label number (0 when empty)."""
    lab, num = label(mask, connectivity)
    if num < 1:
        return mask, (0, 0, -1, 0)
    areas = np.bincount(lab.reshape(-1), minlength=num + 1)[1:]
    win = int(np.argmax(areas)) + 1                                   # first maximum in label order
    out = np.where(lab == win, lab, 0)
    return out, (num, int(areas[win - 1]), int(np.flatnonzero(lab.reshape(-1) == win)[0]), win)
