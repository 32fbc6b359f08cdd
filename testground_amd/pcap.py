"""Captured records (Engine.capture_read, abi.CAPTURE_DTYPE) as a classic pcap file that tcpdump and
Wireshark open: nanosecond timestamps (magic 0xA1B23C4D), LINKTYPE_RAW, headers only.

The engine moves no payload (the bridge keeps the bytes on the host), so each packet is a synthesized
IPv4 + UDP header: addresses from the record's peer ids, total length = the record's `len` (the bytes
on the wire the engine shaped), the simulated time as the timestamp.  The records carry peer ids, not
addresses: a peer that was re-addressed in mid-run (a Config with another IPv4) still appears under
addr_of(peer) for the whole file."""
from __future__ import annotations

import struct
from typing import BinaryIO, Callable, Dict, List

import numpy as np

from . import abi
from . import workloads as wl

MAGIC_NS = 0xA1B23C4D
LINKTYPE_RAW = 101
SNAPLEN = 28  # IPv4 (20 B) + UDP (8 B)
IPPROTO_UDP = 17


def ipv4_checksum(header: bytes) -> int:
    """The Internet checksum of a header whose checksum field is zero (or, over a complete header, 0)."""
    s = sum(struct.unpack(f"!{len(header) // 2}H", header))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def _headers(src_ip: int, dst_ip: int, length: int, ident: int) -> bytes:
    ip = struct.pack("!BBHHHBBHII", 0x45, 0, length, ident & 0xFFFF, 0, 64, IPPROTO_UDP, 0, src_ip, dst_ip)
    ip = ip[:10] + struct.pack("!H", ipv4_checksum(ip)) + ip[12:]
    return ip + struct.pack("!HHHH", 0, 0, max(length - 20, 8), 0)  # ports 0, no UDP checksum


def write_pcap(stream: BinaryIO, records, subnet_base: int = 16 << 24, addr_of: Callable[..., int] = wl.peer_ip,
               refused: bool = False) -> int:
    """Writes `records` (abi.CAPTURE_DTYPE, TX and RX in any order; several arrays may be concatenated)
    merged by (t_ns, dir, src, seq) and returns the packets written.  A TX record whose low verdict
    nibble is not V_SCHEDULED never left its sender (refused, lost or dropped at a full queue): it is left
    out unless refused=True.  Each packet: incl_len = min(28, len) bytes of IPv4 + UDP header, orig_len =
    len, the IP identification = seq & 0xFFFF.  Addresses are addr_of(peer, subnet_base) of the records'
    peer ids, so a mid-run re-addressing is not reflected."""
    r = np.asarray(records, dtype=abi.CAPTURE_DTYPE)
    if not refused:
        r = r[(r["dir"] != abi.CAPTURE_TX) | ((r["verdict"] & 15) == abi.V_SCHEDULED)]
    r = r[np.lexsort((r["seq"], r["src"], r["dir"], r["t_ns"]))]
    stream.write(struct.pack("<IHHiIII", MAGIC_NS, 2, 4, 0, 0, SNAPLEN, LINKTYPE_RAW))
    for x in r:
        t, length = int(x["t_ns"]), int(x["len"])
        src, dst = int(x["src"]), int(x["dst"])
        dst_ip = addr_of(dst, subnet_base) if dst != abi.EXTERNAL else 0xFFFFFFFF
        data = _headers(addr_of(src, subnet_base), dst_ip, length, int(x["seq"]))[:min(SNAPLEN, length)]
        stream.write(struct.pack("<IIII", t // 1_000_000_000, t % 1_000_000_000, len(data), length))
        stream.write(data)
    return len(r)


def read_pcap(stream: BinaryIO) -> List[Dict]:
    """Parses what write_pcap wrote: per packet `t_ns`, `incl_len`, `orig_len` and, where the captured
    bytes hold them, `src_ip`, `dst_ip`, `total_len`, `ident`, `proto`, `checksum_ok`, `udp_len`."""
    head = stream.read(24)
    magic, major, minor, _, _, snaplen, linktype = struct.unpack("<IHHiIII", head)
    if magic != MAGIC_NS or linktype != LINKTYPE_RAW:
        raise ValueError(f"read_pcap: magic {magic:#x}, linktype {linktype}: not a nanosecond LINKTYPE_RAW file")
    out = []
    while True:
        rec = stream.read(16)
        if not rec:
            return out
        if len(rec) != 16:
            raise ValueError("read_pcap: a truncated record header")
        sec, nsec, incl, orig = struct.unpack("<IIII", rec)
        data = stream.read(incl)
        if len(data) != incl or incl > snaplen:
            raise ValueError("read_pcap: a truncated packet")
        p = {"t_ns": sec * 1_000_000_000 + nsec, "incl_len": incl, "orig_len": orig}
        if incl >= 20:
            vihl, _, total, ident, _, _, proto, _, src, dst = struct.unpack("!BBHHHBBHII", data[:20])
            p.update(src_ip=src, dst_ip=dst, total_len=total, ident=ident, proto=proto,
                     checksum_ok=vihl == 0x45 and ipv4_checksum(data[:20]) == 0)
        if incl >= 28:
            p["udp_len"] = struct.unpack("!HHHH", data[20:28])[2]
        out.append(p)
