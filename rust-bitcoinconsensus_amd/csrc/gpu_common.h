// Shared HIP host-side helpers for the engine's kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>

// Return the hipError_t (as int) from the enclosing int-returning function on failure.
#define BCC_HIP_TRY(expr)                                                                   \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            fprintf(stderr, "[bcc] HIP error %d (%s) at %s:%d: %s\n", (int)_e,              \
                    hipGetErrorString(_e), __FILE__, __LINE__, #expr);                      \
            return (int)_e;                                                                 \
        }                                                                                   \
    } while (0)

// Event pairs around spans of one stream's work, for the entries' optional kernel timings: begin(k)
// ... end() adds the span's milliseconds to ms[k] at collect().  With on == false nothing is
// created or recorded.
struct EventSpans {
    bool on;
    double* ms;
    hipStream_t st;
    struct Span {
        hipEvent_t a, b;
        int k;
    };
    std::vector<Span> spans;
    EventSpans(bool on_, double* ms_, hipStream_t st_) : on(on_), ms(ms_), st(st_) {}
    EventSpans(const EventSpans&) = delete;
    EventSpans& operator=(const EventSpans&) = delete;
    void begin(int k) {
        if (!on) return;
        Span s{nullptr, nullptr, k};
        if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
        (void)hipEventRecord(s.a, st);
        spans.push_back(s);
    }
    void end() {
        if (on && !spans.empty()) (void)hipEventRecord(spans.back().b, st);
    }
    void collect() {  // after the stream has been synchronised
        for (Span& s : spans) {
            float t = 0;
            if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) ms[s.k] += t;
        }
    }
    ~EventSpans() {
        for (Span& s : spans) {
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
    }
};
