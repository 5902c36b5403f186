"""Analysis downstream of segmentation (the reference's sequitr/analysis/): neighbours per cell on the GPU.
``analysis.neighbors`` is the module, as in the reference; its ``neighbors()`` is reached through it."""
from . import lineage, linking, neighbors  # noqa: F401
from .neighbors import NeighborTable, label_zones, neighbors_from_objects, zone_graph  # noqa: F401
from .linking import FrameLinker, TrackTable, link_labels, link_pairs, overlap_table, relabel  # noqa: F401
