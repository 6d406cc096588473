// host_stage.h -- device staging of the host-pointer entry points (capi_search.cpp): a bump allocator with a copy list.
//
// The ctx owns ONE device buffer (MatchWs::stage / cap_stage).  A host form declares each piece once -- the host pointer it mirrors and its
// byte count -- and reads "declare, upload, launch, download":
//     HostStage s{c};  auto dq = s.in<float>(q, (size_t)nq * 256);  auto o0 = s.out<int>(best_idx, (size_t)nq * 4);
//     if (const int rc = s.upload(); rc != XFH_OK) return rc;     // select the device, lay out, grow at most once, H2D copies on c->stream
//     HIPCK(c, launch_...(c, dq, ..., o0));                        // a handle converts to its device pointer from upload() on
//     return s.download();                                        // D2H copies on c->stream, ONE hipStreamSynchronize
// Every piece starts on a 256-byte boundary and EVERY piece has at least 16 bytes of slack behind it: descriptor tables, index lists, keypoints
// and byte flags were always staged with that much, and giving it to all pieces is simpler than naming the ones that need it.  in_opt / out_opt
// with a null host pointer: no room, no copy, device pointer nullptr.  A piece of zero bytes has a valid pointer that nothing is copied to or from.
// reserve() may free and reallocate the buffer: that is safe only because every host form ends in download()'s stream synchronise, so
// nothing queued on the stream still uses the old buffer when the next form begins.
#pragma once
#include "capi_internal.h"
#include <stdlib.h>

struct HostStage {
    static const int MAXP = 40; static const size_t SLACK = 16;
    struct Piece { size_t bytes, off; const void* src; void* dst; bool absent; };
    template <typename T> struct Dev { const HostStage* s; int i; operator T*() const { return (T*)s->ptr(i); } };
    xfh_ctx* c; Piece pc[MAXP]; int n = 0;                                   // an aggregate: HostStage s{c};
    template <typename T> Dev<T> add(size_t bytes, const void* src, void* dst, bool absent) {
        if (n == MAXP) abort();                                              // a programming error of the call site, never of the caller
        pc[n] = Piece{bytes, 0, src, dst, absent};
        return Dev<T>{this, n++};
    }
    template <typename T> Dev<T> in(const void* src, size_t bytes) { return add<T>(bytes, src, nullptr, false); }
    template <typename T> Dev<T> in_opt(const void* src, size_t bytes) { return add<T>(bytes, src, nullptr, !src); }
    template <typename T> Dev<T> out(void* dst, size_t bytes) { return add<T>(bytes, nullptr, dst, false); }
    template <typename T> Dev<T> out_opt(void* dst, size_t bytes) { return add<T>(bytes, nullptr, dst, !dst); }
    template <typename T> Dev<T> tmp(size_t bytes) { return add<T>(bytes, nullptr, nullptr, false); }          // device only: grids, workspaces
    void* ptr(int i) const { return pc[i].absent ? nullptr : (char*)c->mws.stage + pc[i].off; }

    // offsets of the pieces -> bytes of the whole (a pure function of the list)
    static size_t layout(Piece* pc, int n) {
        size_t off = 0;
        for (int i = 0; i < n; ++i) { pc[i].off = off; if (!pc[i].absent) off += (pc[i].bytes + SLACK + 255) & ~(size_t)255; }
        return off;
    }
    static int reserve(xfh_ctx* c, size_t need) {
        MatchWs& w = c->mws;
        if (w.stage && w.cap_stage >= need) return XFH_OK;
        if (w.stage) { hipFree(w.stage); w.stage = nullptr; w.cap_stage = 0; }
        HIPCK(c, hipMalloc(&w.stage, need));
        w.cap_stage = need;
        return XFH_OK;
    }
    int upload() {
        HIPCK(c, hipSetDevice(c->cfg.device));
        if (const int rc = reserve(c, layout(pc, n)); rc != XFH_OK) return rc;
        for (int i = 0; i < n; ++i)
            if (pc[i].src && pc[i].bytes) HIPCK(c, hipMemcpyAsync(ptr(i), pc[i].src, pc[i].bytes, hipMemcpyHostToDevice, c->stream));
        return XFH_OK;
    }
    int download() {
        for (int i = 0; i < n; ++i)
            if (pc[i].dst && pc[i].bytes) HIPCK(c, hipMemcpyAsync(pc[i].dst, ptr(i), pc[i].bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        return XFH_OK;
    }
};
