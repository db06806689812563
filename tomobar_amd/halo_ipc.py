"""Device-direct halo transport of the z-slab path: every rank packs its ghost planes into memory it EXPORTS, and its
z-neighbours copy them out of their mapping of that memory (no counterpart in the reference, which never moves data between
its replicas).  ``SlabComm(..., transport="ipc")`` of tomobar_amd/slab.py drives it; docs/multi_gpu.md has the protocol.

Two providers serve the memory, chosen by the device of the tensors:
  * ``HipRegions``: HIP IPC (tomo_ipc_region_* of the library) with tomo_halo_pack2 / tomo_halo_pull2 as the copies -- one
    launch packs both directions, one launch pulls both neighbours' messages;
  * ``ShmRegions``: ``multiprocessing.shared_memory`` with plain slice copies, for host tensors: the CPU tests run the
    whole protocol on it.

The protocol never waits on the device: a kernel neither spins on a flag nor waits for another process's event.  What tells a
neighbour that a message is ready, and an owner that a slot is free again, are small TOKENS sent through the process group
(gloo), so every wait is a host-side receive bounded by the group's time-out.

  post   pack both directions into a free slot of an own region (a new region if none is free or large enough), wait for
         that copy on the host, isend one token to every neighbour this exchange has traffic with: which region (its
         handle), where in it, how many bytes -- and the slots of THAT neighbour this rank has finished reading (the acks
         ride on the tokens).  A post never waits for a peer.
  wait   receive the neighbours' tokens (tokens of later exchanges that arrive first are kept), take the acks they carry,
         map regions not seen before, pull both messages with one launch on the current stream, wait for it on the host and
         note the slots as read.

A boundary with traffic in one direction only still moves a token each way, so acks always come back: both sides know from
their own arguments that the boundary is active (the k-th block sent up by rank r lands in the k-th block of rank r+1's
recv_down)."""

from __future__ import annotations

import ctypes as C
import os
import sys
import time

import torch

SLOTS_PER_REGION = 2     # steady state of one exchange at a time: slot k is acked by the token of exchange k + 1
MAX_ACKS = 6             # acks one token carries; more stay due for the next token
HANDLE_BYTES = 64        # hipIpcMemHandle_t / the padded name of a shared-memory segment
TOKEN_TAG = 0x7401
_HEAD = 8                # seq, ok, region id, slot, offset, bytes, tokens heard from the receiver, number of acks
TOKEN_LEN = _HEAD + 2 * MAX_ACKS + HANDLE_BYTES // 8
SHM_PREFIX = "tomo_halo_"


def _round_up(n: int, m: int) -> int:
    return (int(n) + m - 1) // m * m


def staging_bytes(nbytes) -> int:
    """tomo_halo_staging_bytes: every block starts 16-byte aligned in its message."""
    return sum(_round_up(b, 16) for b in nbytes)


class _Region:
    """One exported or mapped piece of memory: ``addr`` (device address, HipRegions) or ``view`` (uint8 tensor over the
    segment ``shm``, ShmRegions)."""

    def __init__(self, addr=None, shm=None, view=None):
        self.addr, self.shm, self.view = addr, shm, view


class HipRegions:
    """Regions in device memory, exported and mapped with HIP IPC by the library; the copies are the library's kernels."""
    kind = "cuda"
    free_while_mapped = False   # an owner frees a region only when no peer can still read it (IpcTransport.release_local)

    def __init__(self, device):
        from . import _lib as L
        self.L, self.lib = L, L.lib()
        device = torch.device(device)
        self.device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)

    def create(self, nbytes: int):
        base, handle = C.c_void_p(), (C.c_ubyte * HANDLE_BYTES)()
        self.L.check(self.lib.tomo_ipc_region_create(self.device.index, int(nbytes), C.byref(base), handle), self.lib)
        return _Region(addr=int(base.value)), bytes(handle)

    def open(self, handle: bytes):
        mapped = C.c_void_p()
        h = (C.c_ubyte * HANDLE_BYTES).from_buffer_copy(handle)
        self.L.check(self.lib.tomo_ipc_region_open(self.device.index, h, C.byref(mapped)), self.lib)
        return _Region(addr=int(mapped.value))

    def close(self, region):
        self.L.check(self.lib.tomo_ipc_region_close(C.c_void_p(region.addr)), self.lib)

    def destroy(self, region):
        torch.cuda.synchronize(self.device)
        self.L.check(self.lib.tomo_ipc_region_destroy(C.c_void_p(region.addr)), self.lib)

    def _tables(self, msg):
        if msg is None:
            return None, None, 0, C.c_void_p(0)
        tensors, nbytes, region, off = msg
        n = len(tensors)
        return ((C.c_void_p * n)(*[t.data_ptr() for t in tensors]), (C.c_size_t * n)(*[int(b) for b in nbytes]), n,
                C.c_void_p(region.addr + off))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def pack2(self, down, up):
        """``down`` / ``up``: (blocks, their byte counts, the region, the offset of the message in it) or None."""
        a0, b0, n0, m0 = self._tables(down)
        a1, b1, n1, m1 = self._tables(up)
        with torch.cuda.device(self.device):
            self.L.check(self.lib.tomo_halo_pack2(a0, b0, n0, m0, a1, b1, n1, m1, self._stream()), self.lib)

    def pull2(self, down, up):
        a0, b0, n0, m0 = self._tables(down)
        a1, b1, n1, m1 = self._tables(up)
        with torch.cuda.device(self.device):
            self.L.check(self.lib.tomo_halo_pull2(m0, a0, b0, n0, m1, a1, b1, n1, self._stream()), self.lib)

    def host_wait(self):
        """The host waits until the copy just queued on the current stream has finished (an event, not a device sync)."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        ev.synchronize()

    def scratch(self, nbytes: int, value: int):
        return torch.full((nbytes,), value, dtype=torch.uint8, device=self.device)


class ShmRegions:
    """The same operations on named shared-memory segments, for host tensors: the handle is the segment's name, the copies
    are slice copies.  Stands in for HipRegions wherever there is no GPU; not a performance path."""
    kind = "cpu"
    free_while_mapped = True   # unlinking removes the name only; a peer's mapping stays valid until it closes it
    _count = 0

    def __init__(self, device=None):
        self.device = torch.device("cpu")

    def create(self, nbytes: int):
        from multiprocessing import shared_memory
        ShmRegions._count += 1
        name = f"{SHM_PREFIX}{os.getpid()}_{ShmRegions._count}"
        shm = shared_memory.SharedMemory(name=name, create=True, size=int(nbytes))
        return (_Region(shm=shm, view=torch.frombuffer(shm.buf, dtype=torch.uint8, count=int(nbytes))),
                name.encode().ljust(HANDLE_BYTES, b"\0"))

    def open(self, handle: bytes):
        from multiprocessing import shared_memory
        name = handle.rstrip(b"\0").decode()
        try:
            shm = shared_memory.SharedMemory(name=name, track=False)   # the owner unlinks it, not this process's tracker
        except TypeError:   # before Python 3.13 an attached segment is tracked as well; the owner's unlink untracks it
            shm = shared_memory.SharedMemory(name=name)
        return _Region(shm=shm, view=torch.frombuffer(shm.buf, dtype=torch.uint8))

    def close(self, region):
        region.view = None   # the tensor holds an export of shm.buf: it must go first
        region.shm.close()

    def destroy(self, region):
        self.close(region)
        region.shm.unlink()

    @staticmethod
    def _copy(msg, pack):
        if msg is None:
            return
        tensors, nbytes, region, off = msg
        for t, b in zip(tensors, nbytes):
            if pack:
                region.view[off:off + int(b)].copy_(t.reshape(-1).view(torch.uint8))
            else:
                t.reshape(-1).view(torch.uint8).copy_(region.view[off:off + int(b)])
            off += _round_up(b, 16)

    def pack2(self, down, up):
        self._copy(down, True)
        self._copy(up, True)

    def pull2(self, down, up):
        self._copy(down, False)
        self._copy(up, False)

    def host_wait(self):
        pass

    def scratch(self, nbytes: int, value: int):
        return torch.full((nbytes,), value, dtype=torch.uint8)


def provider_for(device):
    """HIP IPC for a CUDA device, shared memory for host tensors."""
    if device is not None and torch.device(device).type == "cuda":
        return HipRegions(device)
    return ShmRegions()


class _Token:
    def __init__(self, fields):
        f = [int(v) for v in fields]
        self.seq, self.ok, self.rid, self.slot, self.offset, self.nbytes, self.heard, n_acks = f[:_HEAD]
        self.acks = [(f[_HEAD + 2 * i], f[_HEAD + 2 * i + 1]) for i in range(n_acks)]
        self.handle = torch.tensor(f[_HEAD + 2 * MAX_ACKS:], dtype=torch.int64).numpy().tobytes()


class _Owned:
    """A region this rank exports: SLOTS_PER_REGION slots of ``slot_bytes``; ``readers[s]`` neighbours still read slot s."""

    def __init__(self, region, handle, slot_bytes):
        self.region, self.handle, self.slot_bytes = region, handle, int(slot_bytes)
        self.readers = [0] * SLOTS_PER_REGION


class IpcTransport:
    """The transport of one SlabComm (its rank, neighbours, process group and statistics) over one provider."""

    def __init__(self, comm):
        self.comm, self.provider = comm, None   # the provider is made inside self_test(): a failure there is a check result
        self.peers = [p for p in (comm.rank - 1, comm.rank + 1) if 0 <= p < comm.world]
        self.owned = {}      # region id -> _Owned
        self.mapped = {}     # (peer, region id) -> _Region
        self.next_rid = 0
        self.send_seq = {p: 0 for p in self.peers}
        self.recv_seq = {p: 0 for p in self.peers}
        self.inbox = {p: {} for p in self.peers}       # tokens that arrived before their exchange was waited for
        self.acks_due = {p: [] for p in self.peers}    # slots of p this rank has read and not yet reported
        self.sends = {p: [] for p in self.peers}       # (seq, request, tensor) of the tokens on their way to p, oldest first
        self.heard = {p: 0 for p in self.peers}        # exchange tokens received from p so far: told to p on every token
        self.closed = False

    # ---- tokens
    def _send_token(self, peer, seq, ok, rid, slot, offset, nbytes, handle):
        due = self.acks_due[peer]
        acks, self.acks_due[peer] = due[:MAX_ACKS], due[MAX_ACKS:]
        fields = [seq, ok, rid, slot, offset, nbytes, self.heard[peer], len(acks)]
        for a in acks:
            fields.extend(a)
        fields.extend([0] * (2 * (MAX_ACKS - len(acks))))
        t = torch.empty(TOKEN_LEN, dtype=torch.int64)
        t[:len(fields)] = torch.tensor(fields, dtype=torch.int64)
        t[len(fields):] = torch.frombuffer(bytearray((handle or b"").ljust(HANDLE_BYTES, b"\0")), dtype=torch.int64)
        self.sends[peer].append((seq, self.comm.dist.isend(t, peer, group=self.comm.group, tag=TOKEN_TAG), t))

    def _settle_sends(self, peer, below=None):
        """Complete the token sends to ``peer`` with a sequence number under ``below`` (None: all of them).  A gloo send
        completes once the neighbour has posted its receive, and gloo does not report that without waiting: so only sends
        the neighbour SAID it has received (the ``heard`` count on its tokens) are waited for -- that wait returns at once,
        however many exchanges are in flight and in whatever order they are waited for."""
        q = self.sends[peer]
        while q and (below is None or q[0][0] < below):
            q.pop(0)[1].wait()

    def _recv_token(self, peer):
        """The next token of ``peer`` (they arrive in the order they were sent); its acks free slots at once."""
        t = torch.empty(TOKEN_LEN, dtype=torch.int64)
        self.comm.dist.recv(t, src=peer, group=self.comm.group, tag=TOKEN_TAG)
        tok = _Token(t.tolist())
        for rid, slot in tok.acks:
            self.owned[rid].readers[slot] -= 1
        if tok.seq >= 0:   # (the send of the check's token, number -1, is settled with the first exchange token)
            self.heard[peer] += 1
            self._settle_sends(peer, tok.heard)
        return tok

    def _token(self, peer, seq):
        box = self.inbox[peer]
        while seq not in box:
            tok = self._recv_token(peer)
            box[tok.seq] = tok
        return box.pop(seq)

    # ---- regions
    def _new_region(self, slot_bytes):
        slot_bytes = _round_up(max(int(slot_bytes), 1), 4096)
        region, handle = self.provider.create(SLOTS_PER_REGION * slot_bytes)
        rid, self.next_rid = self.next_rid, self.next_rid + 1
        self.owned[rid] = _Owned(region, handle, slot_bytes)
        return rid

    def _take_slot(self, nbytes, readers):
        """A slot nobody reads any more that holds ``nbytes``: the smallest such, else the first slot of a new region (the
        sender alone decides about growth; regions that became too small stay until close())."""
        best = None
        for rid, o in self.owned.items():
            if o.slot_bytes >= nbytes and (best is None or o.slot_bytes < self.owned[best[0]].slot_bytes):
                free = [s for s in range(SLOTS_PER_REGION) if o.readers[s] <= 0]
                if free:
                    best = (rid, free[0])
        if best is None:
            best = (self._new_region(nbytes), 0)
        self.owned[best[0]].readers[best[1]] = readers
        return best

    def _map(self, peer, tok):
        key = (peer, tok.rid)
        if key not in self.mapped:
            self.mapped[key] = self.provider.open(tok.handle)
        return self.mapped[key]

    # ---- the collective check after set-up
    def self_test(self):
        """Every rank exports a region, packs a pattern for each neighbour and pulls its neighbours' patterns; a rank whose
        set-up failed still sends its (failed) tokens, so nobody waits for it.  Returns this rank's error text or None --
        the caller agrees on the outcome with all ranks before anyone uses the transport."""
        rank = self.comm.rank
        n, err, rid = 64, None, -1
        try:
            p = self.provider = provider_for(self.comm.device)
            rid = self._new_region(4096)
            region = self.owned[rid].region
            # the pattern for rank-1 at offset 0, the one for rank+1 at offset 256: bytes of value 2 * rank + direction + 1
            msgs = [([p.scratch(n, 2 * rank + d + 1)], [n], region, 256 * d) if peer in self.peers else None
                    for d, peer in enumerate((rank - 1, rank + 1))]
            p.pack2(*msgs)
            p.host_wait()
        except Exception as e:  # noqa: BLE001
            err = f"{type(e).__name__}: {e}"
        for peer in self.peers:
            d = int(peer > rank)
            self._send_token(peer, -1, int(err is None), rid, 0, 256 * d, n, self.owned[rid].handle if err is None else b"")
        toks = {peer: self._recv_token(peer) for peer in self.peers}
        for peer, tok in toks.items():
            if err is not None or not tok.ok:
                continue
            try:
                got = p.scratch(n, 0)
                msg = ([got], [n], self._map(peer, tok), tok.offset)
                p.pull2(msg if peer < rank else None, msg if peer > rank else None)
                p.host_wait()
                want = 2 * peer + int(peer < rank) + 1   # the neighbour below sent it up, the one above sent it down
                if not bool((got == want).all()):
                    raise RuntimeError(f"the check pattern of rank {peer} arrived damaged")
            except Exception as e:  # noqa: BLE001
                err = f"{type(e).__name__}: {e}"
        return err

    # ---- one exchange
    def post(self, send_down, recv_down, send_up, recv_up):
        if self.closed:
            raise RuntimeError("this SlabComm was closed: its IPC regions are gone")
        comm = self.comm
        t_host = time.perf_counter()
        active = []   # (peer, blocks to send, their bytes, blocks to receive, their bytes)
        for peer, snd, rcv in ((comm.rank - 1, send_down, recv_down), (comm.rank + 1, send_up, recv_up)):
            if peer not in self.peers or not (snd or rcv):
                active.append(None)
                continue
            for t in list(snd) + list(rcv):
                if not t.is_contiguous():
                    raise ValueError("halo blocks must be contiguous plane ranges")
                if t.device.type != self.provider.kind:
                    raise ValueError(f"this SlabComm's IPC transport was set up for {self.provider.kind} tensors, "
                                     f"got a block on {t.device}")
            active.append((peer, list(snd), [t.numel() * t.element_size() for t in snd],
                           list(rcv), [t.numel() * t.element_size() for t in rcv]))
        if not any(active):
            return IpcExchange(self, [], None)
        device = next(t.device for a in active if a for t in a[1] + a[3])
        need = [staging_bytes(a[2]) if a else 0 for a in active]
        off_up = _round_up(need[0], 256)
        rid = slot = -1
        base = 0
        if need[0] + need[1] > 0:
            rid, slot = self._take_slot(off_up + need[1], sum(1 for n in need if n > 0))
            o = self.owned[rid]
            base = slot * o.slot_bytes
            msgs = [(a[1], a[2], o.region, base + off) if a and a[1] else None for a, off in zip(active, (0, off_up))]
            self.provider.pack2(*msgs)
            self.provider.host_wait()   # the neighbours may read the slot as soon as they hold the token
        expect = []
        for a, off, nb in zip(active, (0, off_up), need):
            if a is None:
                expect.append(None)
                continue
            peer = a[0]
            self._send_token(peer, self.send_seq[peer], 1, rid if nb else -1, slot, base + off, nb,
                             self.owned[rid].handle if nb else b"")
            self.send_seq[peer] += 1
            expect.append((peer, self.recv_seq[peer], a[3], a[4]))
            self.recv_seq[peer] += 1
            comm.stats["messages"] += int(bool(a[1])) + int(bool(a[3]))
            comm.stats["bytes"] += int(sum(a[2]))
        comm.stats["exchanges"] += 1
        comm.stats["post_host_ms"] += (time.perf_counter() - t_host) * 1e3
        return IpcExchange(self, expect, device)

    def close(self):
        """Collective: every mapper closes its mappings, and after a barrier -- no rank reads a peer's region any more --
        every owner destroys its regions."""
        if self.closed:
            return
        self.closed = True
        for peer in self.peers:   # every token was received: all exchanges have been waited for on all ranks
            self._settle_sends(peer)
        for key in list(self.mapped):
            self.provider.close(self.mapped.pop(key))
        self.comm.barrier()
        for rid in list(self.owned):
            self.provider.destroy(self.owned.pop(rid).region)

    def release_local(self):
        """What a rank can give back on its own (SlabComm.__del__): its mappings, and the regions no peer can still be
        reading -- all of them where freeing leaves a peer's mapping valid (shared memory), else those whose slots are acked."""
        self.closed = True
        if self.provider is None or (sys.is_finalizing() and not self.provider.free_while_mapped):
            return   # at interpreter exit device memory goes back with the process; no HIP call is made that late
        for key in list(self.mapped):
            self.provider.close(self.mapped.pop(key))
        for rid in list(self.owned):
            if self.provider.free_while_mapped or all(r <= 0 for r in self.owned[rid].readers):
                self.provider.destroy(self.owned.pop(rid).region)


class IpcExchange:
    """Handle of one exchange of the IPC transport: wait() receives the neighbours' tokens and pulls their messages."""

    def __init__(self, transport, expect, device):
        self.tr, self.expect, self.device = transport, expect, device

    def wait(self):
        tr, comm = self.tr, self.tr.comm
        if not self.expect:
            return
        t_host = time.perf_counter()
        on_gpu = self.device is not None and self.device.type == "cuda" and comm.timing
        if on_gpu:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
        msgs, read = [], []
        for e in self.expect:
            if e is None:
                msgs.append(None)
                continue
            peer, seq, blocks, nbytes = e
            tok = tr._token(peer, seq)
            if tok.nbytes != staging_bytes(nbytes):   # (also: blocks sent where none are expected, or none where some are)
                raise RuntimeError(f"rank {peer} sent {tok.nbytes} bytes where this rank expects {staging_bytes(nbytes)}: "
                                   "the two sides of a slab boundary disagree about the blocks of an exchange")
            if not blocks:
                msgs.append(None)
                continue
            msgs.append((blocks, nbytes, tr._map(peer, tok), tok.offset))
            read.append((peer, (tok.rid, tok.slot)))
        if read:
            tr.provider.pull2(*msgs)
            tr.provider.host_wait()   # the owner may reuse the slot as soon as it holds the ack
            for peer, key in read:
                tr.acks_due[peer].append(key)
        if on_gpu:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(torch.cuda.current_stream(self.device))
            comm._events.append((e0, e1))
        comm.stats["wait_host_ms"] += (time.perf_counter() - t_host) * 1e3
        self.expect = []
