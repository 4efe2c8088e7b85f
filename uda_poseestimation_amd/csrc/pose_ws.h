// The workspaces of the instance layer, each layout stated once: a struct built from (base, sizes) holds the pointers its launcher hands
// to the kernels and, in `bytes`, what its *_ws_bytes reports (a null base serves for the count).  Plain host C++: a CPU test compiles it.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct WsCarver {      // consecutive regions of one allocation
    uintptr_t base;
    size_t bytes;
    template <typename T>
    T* take(size_t count) {
        T* p = (T*)(base + bytes);
        bytes += count * sizeof(T);
        return p;
    }
    void pad8() { bytes = (bytes + 7) / 8 * 8; }
};

struct PoseNmsWs : WsCarver {      // udapose_pose_nms: the mask [M][ceil(M / 64)], the areas [M], the refused flags [M]
    unsigned long long* mask;
    float* area;
    unsigned char* refused;
    PoseNmsWs(void* b, int M) : WsCarver{(uintptr_t)b, 0} {
        mask = take<unsigned long long>((size_t)M * ((size_t)(M + 63) / 64)), area = take<float>(M), refused = take<unsigned char>(M);
    }
};
struct ApMatchWs : WsCarver {      // udapose_ap_match: the order [M], the ordered frames [M] (-1: refused), the areas [M], the record offsets [F]
    int *order, *ofr, *rec_off;
    float* darea;
    ApMatchWs(void* b, int M, int F) : WsCarver{(uintptr_t)b, 0} {
        order = take<int>(M), ofr = take<int>(M), darea = take<float>(M), rec_off = take<int>(F);
        pad8();
    }
};
struct ApCurveWs : WsCarver {      // udapose_ap_curve: the sorted records (score, matched, ignored) [capacity], the tp and fp counts [T * A][capacity]
    float* ss;
    unsigned long long *sm, *si;
    int *tpc, *fpc;
    ApCurveWs(void* b, int capacity, int T, int A) : WsCarver{(uintptr_t)b, 0} {
        ss = take<float>(capacity);
        pad8();
        sm = take<unsigned long long>(capacity), si = take<unsigned long long>(capacity);
        tpc = take<int>((size_t)T * A * capacity), fpc = take<int>((size_t)T * A * capacity);
    }
};
