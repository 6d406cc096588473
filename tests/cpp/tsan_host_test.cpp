// tsan_host_test.cpp -- the entry points of libxfeat_hip that the headers call "host, stateless, thread-safe", called the way the SLAM threads
// call them: from several threads at once, the FIRST call of the process included.  Compiled with -fsanitize=thread and linked against the
// ThreadSanitizer build of the library's host code (make -C xfeatslam_amd/csrc tsan); run with TSAN_OPTIONS=halt_on_error=1, so a report ends
// the process with a non-zero status.  Eight threads leave one barrier together; each runs `pass` LOOPS times, and no thread has been in the
// library before them.  Afterwards the main thread runs the same pass alone: every pass of every thread must have produced its bytes.
// Needs no GPU and must find none: xfh_create has to fail with XFH_ERR_NO_DEVICE on every thread.
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "xfeat_hip.h"
#include "xfeat_hip_bench.h"
#include "grid_blob.h"

static const int THREADS = 8, LOOPS = 300;

struct Bytes {
    std::vector<unsigned char> v;
    template <class T> void put(const T* p, size_t n) { const unsigned char* b = (const unsigned char*)p; v.insert(v.end(), b, b + n * sizeof(T)); }
    template <class T> void one(T x) { put(&x, 1); }
    void str(const char* s) { put(s, strlen(s) + 1); }
};

struct Inputs {
    xfh_camera cam;
    xfh_grid_bounds img;
    std::vector<float> xy, xyz, normals, dists, desc, ur2;
    std::vector<uint32_t> node_of;
    std::vector<unsigned char> grid;
    float Tcw[12], Ow[3], F12[9], ep[2], sf[8];
    int n = 257;
    Inputs() {
        memset(&cam, 0, sizeof cam);
        cam.fx = 517.3f; cam.fy = 516.5f; cam.cx = 318.6f; cam.cy = 255.3f; cam.k1 = 0.2624f; cam.k2 = -0.9531f; cam.p1 = -0.0054f; cam.p2 = 0.0026f; cam.k3 = 1.1633f;
        cam.bf = 40.0f; cam.width = 640; cam.height = 480;
        img = {0.f, 0.f, 640.f, 480.f};
        unsigned seed = 2024;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
        for (int i = 0; i < n; ++i) {
            xy.push_back(640.f * rnd()); xy.push_back(480.f * rnd());
            const float z = 1.f + 6.f * rnd();
            xyz.push_back((xy[2 * i] - cam.cx) / cam.fx * z); xyz.push_back((xy[2 * i + 1] - cam.cy) / cam.fy * z); xyz.push_back(i % 17 == 0 ? -z : z);
            normals.push_back(0.2f * rnd() - 0.1f); normals.push_back(0.2f * rnd() - 0.1f); normals.push_back(-1.f);
            dists.push_back(0.5f * z); dists.push_back(2.f * z); dists.push_back(1.5f * z);
            ur2.push_back(i % 3 ? -1.f : xy[2 * i] - 40.f / z);
            node_of.push_back(i % 11 == 0 ? XFH_NODE_NONE : (uint32_t)(i % 7) * 0x10000001u);
        }
        for (int i = 0; i < 4 * 64; ++i) desc.push_back(rnd() - 0.5f);
        const float T[12] = {1.f, 0.001f, -0.002f, 0.01f, -0.001f, 1.f, 0.003f, -0.02f, 0.002f, -0.003f, 1.f, 0.03f};
        memcpy(Tcw, T, sizeof T);
        Ow[0] = -0.01f; Ow[1] = 0.02f; Ow[2] = -0.03f;
        const float Fm[9] = {1e-7f, -3e-6f, 8e-4f, 2.5e-6f, 2e-7f, -6e-3f, -9e-4f, 5.5e-3f, 0.1f};
        memcpy(F12, Fm, sizeof Fm);
        ep[0] = 400.f; ep[1] = 250.f;
        sf[0] = 1.f;
        for (int k = 1; k < 8; ++k) sf[k] = sf[k - 1] * 1.2f;
        grid = example_grid_blob();                              // (sized from the layout constants: no call into the library here)
    }
};

// every listed entry point once, all outputs appended to `o`; false: a status was not the expected one
static bool pass(const Inputs& in, Bytes& o) {
    const int n = in.n;
    bool ok = true;
    o.str(xfh_version());
    for (int k = -1; k <= XFH_K_COUNT; ++k) o.str(xfh_kernel_name(k));
    for (int s = -1; s < 14; ++s) o.str(xfh_strerror(s));
    for (int i = 0; i < 3; ++i) o.one(xfh_descriptor_distance(in.desc.data() + 64 * i, in.desc.data() + 64 * (i + 1)));
    std::vector<float> un(2 * n);
    ok &= xfh_undistort_points(&in.cam, in.xy.data(), n, un.data()) == XFH_OK;
    o.put(un.data(), un.size());
    xfh_grid_bounds b = {0, 0, 0, 0};
    ok &= xfh_camera_bounds(&in.cam, &b) == XFH_OK;
    o.put(&b, 1);
    std::vector<float> uvr(3 * n), ur(n);
    std::vector<unsigned char> st(n);
    ok &= xfh_project_points(in.Tcw, &in.cam, &in.img, in.xyz.data(), n, 7.0f, uvr.data(), ur.data(), st.data()) == XFH_OK;
    o.put(uvr.data(), uvr.size()); o.put(ur.data(), ur.size()); o.put(st.data(), st.size());
    float rmax[7];
    ok &= xfh_scale_level_thresholds(1.2f, 8, rmax) == XFH_OK;
    o.put(rmax, 7);
    std::vector<int> lv(n);
    ok &= xfh_fuse_project(in.Tcw, in.Ow, &in.cam, &in.img, 3.0f, in.sf, rmax, 8, in.xyz.data(), in.normals.data(), in.dists.data(), n, uvr.data(), ur.data(), lv.data(),
                           st.data()) == XFH_OK;
    o.put(uvr.data(), uvr.size()); o.put(ur.data(), ur.size()); o.put(lv.data(), lv.size()); o.put(st.data(), st.size());
    for (int flags = 0; flags < 4; ++flags) {
        ok &= xfh_epipolar_gate(in.F12, in.ep, 100.0f, 1.0f, flags, 300.f, 200.f, flags & 1, in.xy.data(), in.ur2.data(), n, st.data()) == XFH_OK;
        o.put(st.data(), st.size());
    }
    for (int best = 0; best < 130; best += 7)
        for (int second = best; second < 300; second += 31) o.one((char)xfh_bow_accept(best % 5 - 1, best, second, 100, 0.6f, best & 1));
    std::vector<unsigned char> blob(xfh_nodes_bytes(n), 0xA5);
    int nn = -1, nn2 = -1;
    ok &= xfh_nodes_pack(in.node_of.data(), n, blob.data(), &nn) == XFH_OK;
    o.put(blob.data(), blob.size()); o.one(nn);
    std::vector<uint32_t> nid(n, 0u);
    std::vector<int> ns(n + 1, 0), items(n, 0);
    ok &= xfh_nodes_unpack(blob.data(), blob.size(), n, nid.data(), ns.data(), items.data(), &nn2) == XFH_OK && nn2 == nn;
    o.put(nid.data(), nid.size()); o.put(ns.data(), ns.size()); o.put(items.data(), items.size());
    std::vector<int> cs(XFH_GRID_COLS * XFH_GRID_ROWS + 1, 0), git(8, 0);
    int nb = -1;
    ok &= xfh_grid_unpack(in.grid.data(), in.grid.size(), 8, cs.data(), git.data(), &nb) == XFH_OK;
    o.put(cs.data(), cs.size()); o.put(git.data(), git.size()); o.one(nb);
    for (int k : {-1, 0, 1, 63, 257, 4096, XFH_GRID_MAX_N}) {
        o.one(xfh_record_bytes(k > 0 ? k : 1)); o.one(xfh_record_desc_offset(k > 0 ? k : 1)); o.one(xfh_match_image_bytes(k)); o.one(xfh_grid_bytes(k));
        o.one(xfh_nodes_bytes(k)); o.one(xfh_compact_bytes_max(k > 0 ? k : 1, 3)); o.one(xfh_search_projection_workspace_bytes(k, 515, 2));
        o.one(xfh_bow_search_workspace_bytes(k, 515, 2));
    }
    o.one(xfh_record_kps_offset());
    xfh_config cfg;
    xfh_config_default(&cfg);
    o.put(&cfg, 1);
    cfg.nfeatures = 64; cfg.max_height = 64; cfg.max_width = 96;
    xfh_ctx* ctx = nullptr;
    const int rc = xfh_create(&cfg, &ctx);
    if (ctx) xfh_destroy(ctx);                                   // (a GPU was found: the status below fails the pass)
    ok &= rc == XFH_ERR_NO_DEVICE && ctx == nullptr;
    o.one(rc);
    return ok;
}

struct Barrier {
    std::mutex m; std::condition_variable cv; int waiting = 0;
    void wait(int n) { std::unique_lock<std::mutex> l(m); if (++waiting == n) cv.notify_all(); else cv.wait(l, [&] { return waiting >= n; }); }
};

int main() {
    const Inputs in;                                             // (no library call: the library is first entered inside the threads)
    Barrier gate;
    std::atomic<int> bad{0};
    std::vector<Bytes> first(THREADS);
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t)
        th.emplace_back([&, t] {
            gate.wait(THREADS);
            for (int k = 0; k < LOOPS && !bad.load(); ++k) {
                Bytes o;
                if (!pass(in, o)) { fprintf(stderr, "tsan_host_test: thread %d pass %d: a status differs\n", t, k); bad = 1; return; }
                if (k == 0) first[t].v.swap(o.v);
                else if (o.v != first[t].v) { fprintf(stderr, "tsan_host_test: thread %d pass %d differs from its first pass\n", t, k); bad = 1; return; }
            }
        });
    for (auto& x : th) x.join();
    if (bad.load()) return 1;
    Bytes serial;
    if (!pass(in, serial)) { fprintf(stderr, "tsan_host_test: the serial pass: a status differs\n"); return 1; }
    for (int t = 0; t < THREADS; ++t)
        if (first[t].v != serial.v) { fprintf(stderr, "tsan_host_test: thread %d differs from the serial pass\n", t); return 1; }
    printf("tsan_host_test ok: %d threads x %d passes, %zu bytes each, equal to the serial pass\n", THREADS, LOOPS, serial.v.size());
    return 0;
}
