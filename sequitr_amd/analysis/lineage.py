"""Lineage trees out of tracks: the binary trees the reference's sequitr/analysis/lineage.py builds from ``parent`` and
``children``, by its breadth-first walk.  Written fresh for Python 3; no matplotlib -- plotting is not built.  Host only."""
from collections import OrderedDict

from ..dataio.tracker import Track


class LineageTreeNode(object):
    """a node of a lineage tree: ``track`` the Track, ``left`` / ``right`` the two daughters, ``depth`` below the root"""

    def __init__(self, track=None, root=False, depth=0):
        if not isinstance(root, bool) or depth < 0:
            raise ValueError("root must be a bool and depth >= 0")
        self.root, self.depth, self.track = root, depth, track
        self.left = self.right = None

    @property
    def leaf(self):
        return self.left is None or self.right is None

    @property
    def children(self):
        return [] if self.leaf else [self.left, self.right]

    @property
    def ID(self):
        return self.track.ID

    @property
    def start(self):
        return self.track.t[0]

    @property
    def end(self):
        return self.track.t[-1]

    def to_dict(self):
        return tree_to_dict(self)


def tree_to_dict(root):
    """the tree from `root` down as nested JSON-compatible dicts: name (the ID as a string), start, end and, for a node
    that divided, children [left, right]"""
    if not isinstance(root, LineageTreeNode):
        raise TypeError("root must be a LineageTreeNode")
    tree = OrderedDict([("name", str(int(root.ID))), ("start", root.start), ("end", root.end)])
    if root.children:
        tree["children"] = [tree_to_dict(root.left), tree_to_dict(root.right)]
    return tree


def linearise_tree(root):
    """the nodes of a tree in breadth-first order"""
    queue, out = [root], []
    while queue:
        node = queue.pop(0)
        out.append(node)
        queue.extend(node.children)
    return out


class LineageTree(object):
    """LineageTree(tracks).create() -> the root nodes, in the order of the tracks' first frames (ties keep the given order).
    A root is a track whose parent is its own ID, 0 or None; a track that is some tree's daughter is not visited again."""

    def __init__(self, tracks):
        if not isinstance(tracks, list) or not all(isinstance(t, Track) for t in tracks):
            raise TypeError("tracks must be a list of Track")
        self.tracks = sorted(tracks, key=lambda t: t.t[0])
        self._by_id = {t.ID: t for t in self.tracks}
        self.trees = []

    def get_track_by_ID(self, ID):
        return self._by_id[ID]

    def create(self):
        used = set()
        self.trees = []
        for trk in self.tracks:
            if id(trk) in used:
                continue
            root = LineageTreeNode(track=trk, root=True)
            used.add(id(trk))
            queue = [root]
            while queue:
                q = queue.pop(0)
                ch = q.track.children
                if ch and len(ch) == 2:
                    q.left = LineageTreeNode(self.get_track_by_ID(ch[0]), depth=q.depth + 1)
                    q.right = LineageTreeNode(self.get_track_by_ID(ch[1]), depth=q.depth + 1)
                    for node in (q.left, q.right):
                        queue.append(node)
                        used.add(id(node.track))
            self.trees.append(root)
        return self.trees

    @property
    def linear_trees(self):
        return [linearise_tree(t) for t in self.trees]
