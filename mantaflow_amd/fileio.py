"""The .uni / .raw container of the reference's fileio/ (iogrids.cpp:36-44, ioparticles.cpp:37-45): a gzip stream of a four-byte magic,
a 288-byte header and the raw element array; a .raw file is the array alone.  Four families share it: 3-D and 4-D grids (the
UniHeader), particle data and particle systems (the UniPartHeader).  What goes into the header's fields, which of them a loader
checks and how the payload becomes an array is the families' own (core.py)."""
import gzip
import io
import struct
import time

# the magics: 3-D grids, 4-D grids, particle data, particle systems, and the particle systems' older format that no reader takes
GRID, GRID4D, PDATA, PARTS, PARTS_V1 = b"MNT3", b"M4T3", b"PD01", b"PB02", b"PB01"
_UNI_HEADER = "<6i252siQ"       # dimX dimY dimZ gridType elementType bytesPerElement info[252] dimT timestamp = 288 B
_UNI_PART_HEADER = "<6i256sQ"   # dim dimX dimY dimZ elementType bytesPerElement info[256] timestamp = 288 B
_LAYOUT = {GRID: _UNI_HEADER, GRID4D: _UNI_HEADER, PDATA: _UNI_PART_HEADER, PARTS: _UNI_PART_HEADER}
INFO = b"mantaflow_amd 0.1 64bit fp1 hip gfx950"


def extension(name):
    """the file name's extension, dot included"""
    if "." not in name:
        raise RuntimeError("file '%s' does not have an extension" % name)
    return name[name.rfind("."):]


def write(name, payload, magic=None, fields=()):
    """a .uni file of that family: `fields` are the header's integers in file order, the six before the info string and for a grid
    dimT after it; the info string and the timestamp (ms) are added here.  Without a magic, a .raw file: the payload alone."""
    with gzip.open(name, "wb", compresslevel=1) as f:
        if magic is not None:
            f.write(magic + struct.pack(_LAYOUT[magic], *fields[:6], INFO, *fields[6:], int(time.time() * 1000)))
        f.write(payload)


class Reader(object):
    """A file read front to back: magic(), header(), payload().  The four loaders differ in when they touch the stream and in what
    they make of a file they cannot open, so the steps are theirs to take.  `whole` (the particle families): the stream is read at
    once, and a file that is not there or is no gzip stream is "can't open file <name>"; otherwise (the grid families) it is read
    piece by piece and the OSError is the caller's."""

    def __init__(self, name, whole=False):
        if whole:
            try:
                with gzip.open(name, "rb") as f:
                    self.f = io.BytesIO(f.read())
            except OSError:
                raise RuntimeError("can't open file " + name)
        else:
            self.f = gzip.open(name, "rb")

    def __enter__(self): return self
    def __exit__(self, *exc): self.f.close()
    def magic(self): return self.f.read(4)

    def header(self, magic, missing):
        """the integers of that family's header, in file order (see write); a stream that ends inside it raises `missing`"""
        layout = _LAYOUT[magic]
        hb = self.f.read(struct.calcsize(layout))
        if len(hb) != struct.calcsize(layout):
            raise RuntimeError(missing)
        h = struct.unpack(layout, hb)
        return h[:6] + h[7:-1]

    def payload(self, nbytes=-1):
        """the next nbytes of the stream, or fewer if it ends; all that is left by default"""
        return self.f.read(nbytes)
