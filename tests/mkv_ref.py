"""A minimal EBML / Matroska reader for the recorder's files, written from the element table of the Matroska
specification (ids below), not from the writer: it walks EBML header, Segment, Info, Tracks and Clusters and returns
what a player needs. Unknown-size Segments and Clusters (live streams, a session that never ended) are read up to the
last complete element."""
import struct

MASTERS = {0x1A45DFA3: "EBML", 0x18538067: "Segment", 0x1549A966: "Info", 0x1654AE6B: "Tracks", 0xAE: "TrackEntry",
           0xE0: "Video", 0x1F43B675: "Cluster"}
UINTS = {0x4286: "EBMLVersion", 0x42F7: "EBMLReadVersion", 0x42F2: "EBMLMaxIDLength", 0x42F3: "EBMLMaxSizeLength",
         0x4287: "DocTypeVersion", 0x4285: "DocTypeReadVersion", 0x2AD7B1: "TimecodeScale", 0xD7: "TrackNumber",
         0x73C5: "TrackUID", 0x83: "TrackType", 0x9C: "FlagLacing", 0x23E383: "DefaultDuration", 0xB0: "PixelWidth",
         0xBA: "PixelHeight", 0xE7: "Timecode"}
STRINGS = {0x4282: "DocType", 0x4D80: "MuxingApp", 0x5741: "WritingApp", 0x86: "CodecID"}
FLOATS = {0x4489: "Duration"}
SIMPLE_BLOCK = 0xA3
# Segment children end an unknown-size Cluster; a Segment of unknown size runs to the end of the file
LEVEL1 = {0x1549A966, 0x1654AE6B, 0x1F43B675}


class Truncated(Exception):
    pass


def _vint(data, at, keep_marker):
    if at >= len(data):
        raise Truncated
    first = data[at]
    if first == 0:
        raise ValueError(f"a variable-length integer longer than 8 bytes at {at}")
    length = 9 - first.bit_length()
    if at + length > len(data):
        raise Truncated
    value = first if keep_marker else first & ((1 << (8 - length)) - 1)
    for b in data[at + 1:at + length]:
        value = (value << 8) | b
    unknown = not keep_marker and value == (1 << (7 * length)) - 1
    return value, at + length, unknown


def _element(data, at):
    """(id, payload start, payload end or None for an unknown size)."""
    ident, at, _ = _vint(data, at, True)
    size, at, unknown = _vint(data, at, False)
    return ident, at, (None if unknown else at + size)


def parse(data):
    """{'header': {...}, 'info': {...}, 'track': {...}, 'blocks': [{'timecode', 'track', 'flags', 'data'}],
    'clusters': [{'timecode', 'size_known', 'blocks'}], 'segment_size_known', 'complete'}.
    `complete` is False when the file ends inside an element (the blocks before it are returned)."""
    out = {"header": {}, "info": {}, "track": {}, "blocks": [], "clusters": [], "segment_size_known": None, "complete": True}

    def leaf(ident, a, b, into):
        if ident in UINTS:
            into[UINTS[ident]] = int.from_bytes(data[a:b], "big")
        elif ident in STRINGS:
            into[STRINGS[ident]] = data[a:b].decode("ascii")
        elif ident in FLOATS:
            into[FLOATS[ident]] = struct.unpack(">d" if b - a == 8 else ">f", data[a:b])[0]

    def walk(a, b, into, stop_at_level1=False):
        """Children of a master spanning [a, b); returns where it stopped."""
        at = a
        while at < b:
            ident, pa, pe = _element(data, at)
            if stop_at_level1 and ident in LEVEL1:
                return at
            if pe is not None and pe > len(data):
                raise Truncated
            if ident == 0x1F43B675:
                cluster = {"timecode": None, "size_known": pe is not None, "blocks": 0}
                out["clusters"].append(cluster)
                at = walk(pa, pe if pe is not None else b, cluster, stop_at_level1=pe is None)
            elif ident == SIMPLE_BLOCK:
                track, p, _ = _vint(data, pa, False)
                rel = struct.unpack(">h", data[p:p + 2])[0]
                out["blocks"].append({"timecode": into["timecode"] + rel, "track": track, "flags": data[p + 2],
                                      "data": bytes(data[p + 3:pe])})
                into["blocks"] += 1
                at = pe
            elif ident in MASTERS:
                name = MASTERS[ident]
                target = {"EBML": out["header"], "Info": out["info"]}.get(name, out["track"] if name in ("TrackEntry", "Video") else into)
                if name == "Segment":
                    out["segment_size_known"] = pe is not None
                at = walk(pa, pe if pe is not None else len(data), target)
            else:
                if ident == 0xE7:
                    into["timecode"] = int.from_bytes(data[pa:pe], "big")
                else:
                    leaf(ident, pa, pe, into)
                at = pe
        return at

    try:
        walk(0, len(data), {})
    except Truncated:
        out["complete"] = False
    return out
