// Host-side C++ check of include/SVGF.h over a real sequence: drives gpupt::svgfDenoiser the way application::Render drives its
// filter stages (src/App.cu:552-556), with this frame's and the previous frame's G-buffers distinct, and writes every frame's result
// and history for tests/test_gpu_camera_motion.py to compare.  Built with g++ (no device code on the host side).
//   shim_sequence <dir> <W> <H> <frames> <storage: 0 = F32, 1 = F16>
// reads <dir>/{motion,normal,uv,radiance}_<k>.bin (raw planes; radiance already in the storage type), writes <dir>/{out,hist}_<k>.bin.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "SVGF.h"

static std::vector<char> slurp(const std::string& path, size_t bytes) {
    std::vector<char> v(bytes);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), 1, bytes, f) != bytes) throw std::runtime_error("cannot read " + path);
    std::fclose(f);
    return v;
}

static void spill(const std::string& path, const void* data, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, bytes, f) != bytes) throw std::runtime_error("cannot write " + path);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: shim_sequence dir W H frames storage\n"); return 2; }
    const std::string dir = argv[1];
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), N = std::atoi(argv[4]), storage = std::atoi(argv[5]) ? SVGF_F16 : SVGF_F32;
    const size_t px = size_t(W) * H, c4 = storage == SVGF_F16 ? 8 : 16;
    try {
        gpupt::svgfDenoiser den(W, H, storage);
        den.SpatialFilterSteps = 5;
        std::vector<std::unique_ptr<gpupt::buffer>> planes;
        std::vector<svgf_gbuffer> gb;
        for (int k = 0; k < N; k++) {
            const std::string s = "_" + std::to_string(k) + ".bin";
            auto m = slurp(dir + "/motion" + s, px * 16), n = slurp(dir + "/normal" + s, px * 8), u = slurp(dir + "/uv" + s, px * 8);
            planes.emplace_back(new gpupt::buffer(m.size(), m.data()));
            planes.emplace_back(new gpupt::buffer(n.size(), n.data()));
            planes.emplace_back(new gpupt::buffer(u.size(), u.data()));
            gb.push_back(svgf_gbuffer{planes[3 * k]->Data, planes[3 * k + 1]->Data, planes[3 * k + 2]->Data});
        }
        std::vector<char> out(px * c4);
        std::vector<uint8_t> hist(px);
        for (int k = 0; k < N; k++) {
            auto rad = slurp(dir + "/radiance_" + std::to_string(k) + ".bin", px * c4);
            den.Buffers.ColourBuffer->updateData(rad.data(), rad.size());        // the path tracer's output (PathTrace.cuh:618)
            den.TemporalFilter(gb[k], gb[k > 0 ? k - 1 : 0]);
            den.FilterMoments(gb[k]);
            void* result = den.WaveletFilter(gb[k]);
            if (hipMemcpy(out.data(), result, out.size(), hipMemcpyDeviceToHost) != hipSuccess) return 3;
            if (hipMemcpy(hist.data(), den.Buffers.HistoryLength[den.PingPongInx]->Data, px, hipMemcpyDeviceToHost) != hipSuccess) return 3;
            den.EndFrame();
            spill(dir + "/out_" + std::to_string(k) + ".bin", out.data(), out.size());
            spill(dir + "/hist_" + std::to_string(k) + ".bin", hist.data(), hist.size());
        }
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("sequence ok\n");
    return 0;
}
