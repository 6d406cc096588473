// threads_test.cpp -- the C++ layer the SLAM threads call (include/xfeat/ORBmatcher_xfeat.h) from three std::threads at once, as the reference
// runs it (src/System.cc:197,214,233): each thread has a ctx of its own and builds its OWN XFmatcher for every call, the way LocalMapping.cc and
// LoopClosing.cc build `ORBmatcher matcher(...)`; between two calls it asks the static DescriptorDistance for fixed rows.
//   thread 0  searchByBoW, frame form           (Tracking)
//   thread 1  searchForTriangulation            (LocalMapping)
//   thread 2  searchByBoW, keyframe form        (LoopClosing)
// Every answer is computed once, serially, before a thread exists; every iteration of every thread must reproduce it byte for byte.  The first
// difference or status sets a stop flag that all threads read before each call, and the exit status is non-zero.  The serial answers are written
// out in the formats of bow_test.cpp / triangulation_test.cpp (one dump each), for the driver to compare with the restatements.
// usage: threads_test bow_frame_in.bin triangulation_in.bin bow_keyframe_in.bin out_prefix rounds     (the in.bin formats of bow_test.cpp, triangulation_test.cpp)
#define XFEAT_NO_OPENCV 1
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "xfeat/XFextractor.h"
#include "xfeat/ORBmatcher_xfeat.h"

using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static void put(std::vector<int>& o, const std::vector<T>& v) { for (const T& x : v) o.push_back((int)x); }

struct BowProblem {
    int n1 = 0, n2 = 0; bool keyframe = false; float ratio = 0.f;
    XFmatcher::Mat desc1, desc2;
    std::vector<uint32_t> node1, node2;
    std::vector<unsigned char> flag1, flag2;
    bool read(const char* path) {
        FILE* f = fopen(path, "rb");
        int hdr[4];
        if (!f || !rd(f, hdr, 4) || !rd(f, &ratio, 1)) return false;
        n1 = hdr[0]; n2 = hdr[1]; keyframe = hdr[2] != 0;
        desc1 = XFmatcher::Mat(n1, 64, 4); node1.resize(n1); flag1.resize(n1); desc2 = XFmatcher::Mat(n2, 64, 4); node2.resize(n2); flag2.resize(n2);
        const bool ok = rd(f, desc1.ptr<float>(0), (size_t)n1 * 64) && rd(f, node1.data(), n1) && rd(f, flag1.data(), n1) &&
                        rd(f, desc2.ptr<float>(0), (size_t)n2 * 64) && rd(f, node2.data(), n2) && rd(f, flag2.data(), n2);
        fclose(f);
        return ok;
    }
    // one call on a matcher of its own -> the dump of bow_test.cpp
    std::vector<int> run(xfh_ctx* ctx) const {
        XFmatcher matcher(ctx, ratio, true);
        std::vector<int> mq(3, 9), aq(5, 9), o;
        o.push_back(matcher.searchByBoW(desc1, node1, flag1, desc2, node2, flag2, keyframe, mq, aq));
        put(o, matcher.lastBoWStatus()); put(o, mq); put(o, matcher.lastBoWBestDist()); put(o, matcher.lastBoWSecondDist()); put(o, matcher.lastBoWCandidates()); put(o, aq);
        return o;
    }
};

struct TriProblem {
    int n1 = 0, n2 = 0, flags = 0;
    xfh_camera cam; float F12[9], ep[2];
    struct KF { XFmatcher::Mat desc; std::vector<float> xy, uright; std::vector<unsigned char> has; std::vector<uint32_t> node_of; } k[2];
    bool read(const char* path) {
        FILE* f = fopen(path, "rb");
        int hdr[4];
        if (!f || !rd(f, hdr, 4) || !rd(f, &cam, 1) || !rd(f, F12, 9) || !rd(f, ep, 2)) return false;
        n1 = hdr[0]; n2 = hdr[1]; flags = hdr[2];
        bool ok = true;
        for (int s = 0; s < 2 && ok; ++s) {
            const int n = s ? n2 : n1;
            std::vector<XFgrid::KeyPoint> keys(n);
            std::vector<float> depth((size_t)cam.width * cam.height);                 // (the device form's image: read past it)
            k[s].desc = XFmatcher::Mat(n, 64, 4); k[s].uright.resize(n); k[s].has.resize(n); k[s].node_of.resize(n); k[s].xy.resize(2 * (size_t)n);
            ok = rd(f, keys.data(), n) && rd(f, k[s].desc.ptr<float>(0), (size_t)n * 64) && rd(f, k[s].uright.data(), n) && rd(f, k[s].has.data(), n) &&
                 rd(f, k[s].node_of.data(), n) && rd(f, depth.data(), depth.size());
            for (int i = 0; i < n && ok; ++i) { k[s].xy[2 * i] = keys[i].pt.x; k[s].xy[2 * i + 1] = keys[i].pt.y; }
        }
        fclose(f);
        return ok;
    }
    // one call on a matcher of its own -> the dump of triangulation_test.cpp
    std::vector<int> run(xfh_ctx* ctx) const {
        XFmatcher matcher(ctx, 0.6f, false);
        std::vector<std::pair<size_t, size_t>> pairs(3, std::make_pair((size_t)9, (size_t)9));
        std::vector<int> o;
        o.push_back(matcher.searchForTriangulation(k[0].desc, k[0].xy, &k[0].uright, k[0].has, k[0].node_of, k[1].desc, k[1].xy, &k[1].uright, k[1].has, k[1].node_of, F12, ep,
                                                   pairs, (flags & 1) != 0, (flags & 2) != 0));
        o.push_back((int)pairs.size());
        for (const auto& pr : pairs) { o.push_back((int)pr.first); o.push_back((int)pr.second); }
        put(o, matcher.lastTriangulationStatus()); put(o, matcher.lastTriangulationMatches()); put(o, matcher.lastTriangulationBestDist());
        put(o, matcher.lastTriangulationCandidates()); put(o, matcher.lastTriangulationGeom());
        return o;
    }
};

// the static member on fixed rows of the first problem: the same 16 integers whoever asks
static std::vector<int> distances(const BowProblem& b) {
    std::vector<int> o;
    for (int i = 0; i < 16; ++i) {
        XFmatcher::Mat a(1, 64, 4), c(1, 64, 4);
        memcpy(a.ptr<float>(0), b.desc1.ptr<float>(0) + 64 * (size_t)((7 * i) % b.n1), 256);
        memcpy(c.ptr<float>(0), b.desc2.ptr<float>(0) + 64 * (size_t)((11 * i) % b.n2), 256);
        o.push_back(XFmatcher::DescriptorDistance(a, c));
    }
    return o;
}

static bool write(const std::string& path, const std::vector<int>& v) {
    FILE* o = fopen(path.c_str(), "wb");
    if (!o) return false;
    const bool ok = fwrite(v.data(), 4, v.size(), o) == v.size();
    return fclose(o) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
    BowProblem bow[2]; TriProblem tri;
    if (!bow[0].read(argv[1]) || !tri.read(argv[2]) || !bow[1].read(argv[3]) || bow[0].keyframe || !bow[1].keyframe) return 2;
    const std::string prefix = argv[4];
    const int rounds = atoi(argv[5]);
    xfh_ctx* ctx[3] = {nullptr, nullptr, nullptr};
    int status = 0;
    try {
        xfh_config cfg; xfh_config_default(&cfg);
        cfg.nfeatures = 1; cfg.max_height = 32; cfg.max_width = 32;
        for (int t = 0; t < 3; ++t) if (xfh_create(&cfg, &ctx[t]) != XFH_OK) return 4;
        // 1. every answer once, serially
        const std::vector<int> want[3] = {bow[0].run(ctx[0]), tri.run(ctx[1]), bow[1].run(ctx[2])};
        const std::vector<int> want_dist = distances(bow[0]);
        if (!write(prefix + "_bow_frame.bin", want[0]) || !write(prefix + "_triangulation.bin", want[1]) || !write(prefix + "_bow_keyframe.bin", want[2])) return 3;
        // 2. three threads, released together
        std::atomic<bool> stop{false};
        std::atomic<int> failed{0};
        std::mutex m; std::condition_variable cv; int waiting = 0;
        std::vector<std::thread> th;
        for (int t = 0; t < 3; ++t)
            th.emplace_back([&, t] {
                { std::unique_lock<std::mutex> l(m); if (++waiting == 3) cv.notify_all(); else cv.wait(l, [&] { return waiting >= 3; }); }
                try {
                    for (int it = 0; it < rounds; ++it) {
                        if (stop.load()) return;
                        const std::vector<int> got = t == 0 ? bow[0].run(ctx[0]) : t == 1 ? tri.run(ctx[1]) : bow[1].run(ctx[2]);
                        if (got != want[t]) { stop = true; failed |= 1 << t; fprintf(stderr, "thread %d iteration %d: the answer differs from the serial one\n", t, it); return; }
                        if (stop.load()) return;
                        if (distances(bow[0]) != want_dist) { stop = true; failed |= 1 << t; fprintf(stderr, "thread %d iteration %d: DescriptorDistance differs\n", t, it); return; }
                    }
                } catch (const std::exception& e) { stop = true; failed |= 8 << t; fprintf(stderr, "thread %d: %s\n", t, e.what()); }
            });
        for (auto& x : th) x.join();
        if (failed.load()) status = 6;
        else printf("threads_test ok: 3 threads x %d iterations\n", rounds);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); status = 5; }
    if (status == 0) for (int t = 0; t < 3; ++t) xfh_destroy(ctx[t]);          // (after a failure nothing more is asked of the GPU)
    return status;
}
