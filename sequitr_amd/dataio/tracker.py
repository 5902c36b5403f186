"""Tracks as the reference's analysis modules consume them: a ``Track`` with the attribute names of
sequitr/dataio/tracker.py and the JSON layout its read_JSON opens.  Written fresh for Python 3; only the field names and
the file layout are the interface.  Host only.

Layout: ``<folder>/tracks_<cell_type>.json`` = {cell_type: {"files": [...], "path": folder, "zipped": bool}} and one JSON
document per track -- inside ``<folder>/tracks_<cell_type>.zip`` when zipped, next to the index otherwise.  A track's
document holds ID, x, y, z, t, length, label (the object's class at every frame), parent, children, fate and
neighborhood; ``cell_type`` and ``filename`` are filled in by read_JSON, as in the reference.  Tracker XML is not built."""
import json
import os
import zipfile

FIELDS = ('ID', 'x', 'y', 'z', 't', 'length', 'label', 'parent', 'children', 'fate', 'neighborhood')


class Track(object):
    """One cell followed through the movie: ``t`` the frames, ``x`` / ``y`` / ``z`` the centre per frame, ``label`` the
    class per frame, ``parent`` the ID of the track that divided into this one (a root's own ID), ``children`` [] or the two
    IDs it divided into."""

    def __init__(self, ID=None):
        self.ID = ID
        self.x = self.y = self.z = self.t = None
        self.length = None
        self.label = None
        self.parent = None
        self.children = []
        self.fate = None
        self.cell_type = None
        self.neighborhood = []
        self.filename = None

    @property
    def n(self):
        return self.t

    def in_frame(self, frame):
        """whether the track is present in `frame`"""
        return frame in self.t

    def __len__(self):
        return self.length

    def to_dict(self):
        return {name: getattr(self, name) for name in FIELDS}

    @staticmethod
    def from_dict(params):
        T = Track()
        for k, v in params.items():
            setattr(T, k, v)
        return T


def _track_filename(track, cell_type):
    return "track_%d_%s.json" % (int(track.ID), cell_type)


def write_JSON(folder, tracks, cell_type, zipped=True):
    """write `tracks` in the layout of the module's text; returns the index file's path"""
    os.makedirs(folder, exist_ok=True)
    files = [_track_filename(t, cell_type) for t in tracks]
    if zipped:
        with zipfile.ZipFile(os.path.join(folder, "tracks_%s.zip" % cell_type), 'w', zipfile.ZIP_DEFLATED) as z:
            for fn, t in zip(files, tracks):
                z.writestr(fn, json.dumps(t.to_dict()))
    else:
        for fn, t in zip(files, tracks):
            with open(os.path.join(folder, fn), 'w') as f:
                json.dump(t.to_dict(), f)
    index = os.path.join(folder, "tracks_%s.json" % cell_type)
    with open(index, 'w') as f:
        json.dump({cell_type: {"files": files, "path": folder, "zipped": bool(zipped)}}, f, indent=2)
    return index


def read_JSON(folder, cell_type):
    """the tracks write_JSON (or the reference's exporter) left in `folder`, in the index's order"""
    index = os.path.join(folder, "tracks_%s.json" % cell_type)
    if not os.path.exists(index):
        raise IOError("Tracking data file not found: %s" % index)
    with open(index) as f:
        entry = json.load(f)[cell_type]
    tracks = []

    def add(fn, text):
        d = json.loads(text)
        d['cell_type'], d['filename'] = cell_type, fn
        tracks.append(Track.from_dict(d))

    if entry.get('zipped'):
        with zipfile.ZipFile(os.path.join(folder, "tracks_%s.zip" % cell_type)) as z:
            for fn in entry['files']:
                add(fn, z.read(fn).decode())
    else:
        for fn in entry['files']:
            with open(os.path.join(folder, fn)) as f:
                add(fn, f.read())
    return tracks
