"""``generate_boundary`` (reference: min_path_processing/utils.py:4-18): label map -> first row of each
region, per column.  Boundaries belong to the first pixel of the "next" region."""
import numpy as np


def generate_boundary(img_array, axis=0):
    num_classes = int(np.amax(img_array))
    return np.array([np.argmax(img_array == i, axis=axis) for i in range(1, num_classes + 1)])


def generate_boundary_masked(labels, num_classes, ignore_label, axis=0):
    """``generate_boundary`` for partially labelled maps (extension; no counterpart in the reference): always
    ``num_classes - 1`` boundaries.  For boundary i and a line along ``axis`` (a column of the image), with r the first
    position whose label is i: r if no position 0..r of that line carries ``ignore_label``, else 0 -- what lies under an
    unknown pixel has no known depth.  Where class i does not occur the result is 0, as ``argmax`` gives there.  On maps
    without the ignore label in which class ``num_classes - 1`` occurs it equals ``generate_boundary``."""
    labels = np.asarray(labels)
    first = np.array([np.argmax(labels == i, axis=axis) for i in range(1, int(num_classes))])
    ignored = labels == ignore_label
    first_ignored = np.where(ignored.any(axis=axis), np.argmax(ignored, axis=axis), labels.shape[axis])
    return np.where(first < first_ignored[None], first, 0)
