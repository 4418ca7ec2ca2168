// The staged call of a host-buffer entry (host code), built on the pieces of workspace.h: what the
// signing, Merkle, trie and ingress entries outside the verification hot path copy up, enqueue on and
// copy down through. It needs the runtime's copies and synchronisation on top of what workspace.h uses.
#ifndef PV_STAGE_H
#define PV_STAGE_H

#include <string.h>

#include <algorithm>
#include <vector>

#include "workspace.h"

// One staged call of a host-buffer entry: the site lists its sections (each laid out by PvLayout, so
// 256-byte aligned and never empty), upload() grows the blocks and copies the inputs up, dev() gives the
// typed device pointers for the enqueue, download() copies the results down and synchronises. A section
// is named by the int its call returns; -1 names no section and dev(-1) is null (an output the caller
// does not take). Two modes:
//   caller memory: one copy per non-empty input section straight from the caller's pointer into d_in,
//                  one per non-empty output with a dst from d_out straight into the caller's pointer;
//   pinned:        the inputs packed into h, the outputs laid out behind them, d_in a mirror of h: one
//                  copy up over the inputs, one down over the outputs, then a memcpy to each dst.
// Slack is reserved behind a section and not copied in caller-memory mode (kernels read ahead of a blob's
// last byte). Arrays the stage rebases or lends (in_offsets, in_u64) are its own, do not move once handed
// out and live until the next reset(). A stage belongs to a workspace and is reused call after call and
// chunk after chunk: a use that fails between upload() and the end of download() leaves it `busy`, and
// the next reset() synchronises the stream before anything is written again. No destructor, as PvOwner.
struct PvStage {
    PvDevBuf d_in, d_out;
    PvPinnedBuf h;

    // The stage emptied for a use on `s`.
    int reset(hipStream_t s, bool pinned) {
        if (busy) PV_HIP(hipStreamSynchronize(stream), PV_ERR_LAUNCH);
        busy = false;
        stream = s;
        pin = pinned;
        secs.clear();
        li = lo = PvLayout();
        lent = 0;
        return PV_OK;
    }
    // `bytes` at src, copied up, and `slack` more reserved.
    int in(const void* src, uint64_t bytes, uint64_t slack = 0) {
        return add({li.add(bytes + slack), bytes, src, nullptr, false});
    }
    // An array of `count` words the site fills itself before upload(); *sec names its section.
    uint64_t* in_u64(uint64_t count, int* sec) {
        if (lent == own.size()) own.emplace_back();
        std::vector<uint64_t>& v = own[lent++];
        v.resize(count);
        *sec = in(v.data(), 8 * count);
        return v.data();
    }
    // off[0..count] moved to the bytes that are copied: every entry minus off[0].
    int in_offsets(const uint64_t* off, uint64_t count) {
        int sec;
        uint64_t* v = in_u64(count + 1, &sec);
        for (uint64_t i = 0; i <= count; i++) v[i] = off[i] - off[0];
        return sec;
    }
    // `bytes` the kernels write, copied down to dst by download() (dst null: device scratch), and `slack`
    // more reserved (verdict bits are stored as whole words).
    int out(void* dst, uint64_t bytes, uint64_t slack = 0) {
        return add({lo.add(bytes + slack), bytes, nullptr, dst, true});
    }
    // Both: copied up from src, worked on in place, copied down to dst.
    int inout(const void* src, void* dst, uint64_t bytes) { return add({li.add(bytes), bytes, src, dst, false}); }

    int upload() {
        const uint64_t all = li.at + lo.at;
        busy = true;  // until download() has synchronised
        if (int rc = d_in.grow(pin ? all : li.at)) return rc;
        if (int rc = pin ? h.grow(all, hipHostMallocDefault) : d_out.grow(lo.at)) return rc;
        for (const Sec& c : secs) {
            if (!c.src || !c.bytes) continue;
            if (pin) memcpy(h.p + c.off, c.src, c.bytes);
            else PV_HIP(hipMemcpyAsync(d_in.p + c.off, c.src, c.bytes, hipMemcpyHostToDevice, stream), PV_ERR_LAUNCH);
        }
        if (pin && li.at) PV_HIP(hipMemcpyAsync(d_in.p, h.p, li.at, hipMemcpyHostToDevice, stream), PV_ERR_LAUNCH);
        return PV_OK;
    }
    // Valid after upload().
    template <class T>
    T* dev(int sec) const {
        return sec < 0 ? nullptr : reinterpret_cast<T*>(devp(secs[sec]));
    }
    // Pinned mode, after download(): the section's bytes in h.
    const uint8_t* host(int sec) const { return h.p + at(secs[sec]); }
    uint64_t in_bytes() const { return li.at; }

    int download() {
        uint64_t from = li.at;  // pinned: one copy from the first section that goes down to the end
        for (const Sec& c : secs) {
            if (!c.dst || !c.bytes) continue;
            if (pin) from = std::min(from, at(c));
            else PV_HIP(hipMemcpyAsync(c.dst, devp(c), c.bytes, hipMemcpyDeviceToHost, stream), PV_ERR_LAUNCH);
        }
        const uint64_t down = li.at + lo.at - from;
        if (pin && down) PV_HIP(hipMemcpyAsync(h.p + from, d_in.p + from, down, hipMemcpyDeviceToHost, stream), PV_ERR_LAUNCH);
        PV_HIP(hipStreamSynchronize(stream), PV_ERR_LAUNCH);
        busy = false;
        for (const Sec& c : secs)
            if (pin && c.dst && c.bytes) memcpy(c.dst, h.p + at(c), c.bytes);
        return PV_OK;
    }
    void release() {
        d_in.release();  // hipFree synchronises
        d_out.release();
        h.release();
        busy = false;
    }

private:
    struct Sec {
        uint64_t off, bytes;  // off within the inputs, or within the outputs
        const void* src;
        void* dst;
        bool is_out;
    };
    // where a section lies in h and in its device block: pinned mode lays the outputs behind the inputs
    uint64_t at(const Sec& c) const { return c.is_out && pin ? li.at + c.off : c.off; }
    uint8_t* devp(const Sec& c) const { return (c.is_out && !pin ? d_out.p : d_in.p) + at(c); }
    int add(const Sec& c) {
        secs.push_back(c);
        return (int)secs.size() - 1;
    }
    std::vector<Sec> secs;
    std::vector<std::vector<uint64_t>> own;  // the first `lent` are handed out
    size_t lent = 0;
    PvLayout li, lo;
    hipStream_t stream = nullptr;
    bool pin = false, busy = false;
};

#endif  // PV_STAGE_H
