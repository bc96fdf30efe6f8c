// The HRNet graph's kernel selection (csrc/kernel_select.h) on the HOST, with no device and no
// HIP runtime: reads queries from stdin, one per line,
//     route cin cout h w ks stride relu res f32_out cat  batch cus has_image  [switch ...]
// (switch: a Switches field name, or s2_tile=N) and prints for each
//     <kernel below one crop per CU> <kernel from there on> <kernel at this batch> <weight image elements>
// (kernel_name(), "tblock64_kernel:tiles" for tblock64_kernel's strided form, "none" for K_NONE).
// A line that starts with "det" asks the person detector's selection (csrc/det_select.h) instead:
//     det kind h w cin cout ks stride live res fold cus  [switch=value ...]
// (kind: MVP_DET_*; fold: DetFold; switch: a DetSwitches field, e.g. band=4 pers=0 halo_rows2=1)
// and prints
//     <variant> <weight image elements>
// (det_kernel_name(), "none" for DK_NONE).
// tests/test_kernel_select.py builds it with the host compiler and holds the expected answers.
//   c++ -std=c++17 -O1 -Imulti-camera_3d_pose_estimation_amd/csrc tools/kernel_select_check.cpp -o kernel_select_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "det_select.h"
#include "kernel_select.h"

// one "det" query (the stream stands after the word); false: malformed
static bool det_query(std::istringstream& in) {
    using namespace mvp;
    DetOpShape c;
    int fold, cus;
    if (!(in >> c.kind >> c.h >> c.w >> c.cin >> c.cout >> c.ks >> c.stride >> c.live >> c.res >> fold >> cus)) return false;
    DetSwitches sw;
    for (std::string w; in >> w;) {
        const size_t eq = w.find('=');
        if (eq == std::string::npos) return false;
        const std::string name = w.substr(0, eq);
        const int v = atoi(w.c_str() + eq + 1);
        if (name == "xcd") sw.xcd = v;
        else if (name == "band") sw.band = v;
        else if (name == "pers") sw.pers = v;
        else if (name == "pers_occ") sw.pers_occ = v;
        else if (name == "fold") sw.fold = v;
        else if (name == "halo_pers") sw.halo_pers = v;
        else if (name == "halo_rows2") sw.halo_rows2 = v;
        else if (name == "live") sw.live = v;
        else if (name == "head_direct") sw.head_direct = v;
        else return false;
    }
    const DetKernel k = select_det_kernel(c, (DetFold)fold, sw, cus);
    printf("%s %ld\n", k == DK_NONE ? "none" : det_kernel_name(k), det_image_elems(k, c));
    return true;
}

int main() {
    using namespace mvp;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (line.rfind("det ", 0) == 0) {
            std::string word;
            in >> word;
            if (!det_query(in)) {
                fprintf(stderr, "bad detector query: %s\n", line.c_str());
                return 2;
            }
            continue;
        }
        int route, batch, cus, has_image;
        LaunchShape c;
        if (!(in >> route >> c.cin >> c.cout >> c.h >> c.w >> c.ks >> c.stride >> c.relu >> c.res >> c.f32_out >> c.cat >>
              batch >> cus >> has_image))
            continue;
        Switches sw;
        const struct {
            const char* name;
            bool Switches::*field;
        } flags[] = {{"no_fuse", &Switches::no_fuse},           {"no_catfuse", &Switches::no_catfuse},
                     {"no_pairfuse", &Switches::no_pairfuse},   {"no_bneck", &Switches::no_bneck},
                     {"no_stemfuse", &Switches::no_stemfuse},   {"no_transfuse", &Switches::no_transfuse},
                     {"no_sibfuse", &Switches::no_sibfuse},     {"no_headfuse", &Switches::no_headfuse},
                     {"no_tblock64", &Switches::no_tblock64},   {"no_head1x1", &Switches::no_head1x1},
                     {"no_tconv", &Switches::no_tconv},         {"no_tconv16", &Switches::no_tconv16},
                     {"no_s2conv", &Switches::no_s2conv},       {"no_tblock", &Switches::no_tblock},
                     {"no_tblock32s", &Switches::no_tblock32s}, {"stem2_tile", &Switches::stem2_tile},
                     {"crop_stream", &Switches::crop_stream}};
        for (std::string w; in >> w;) {
            bool known = w.rfind("s2_tile=", 0) == 0;
            if (known) sw.s2_tile = atoi(w.c_str() + 8);
            for (const auto& f : flags)
                if (w == f.name) sw.*f.field = known = true;
            if (!known) {
                fprintf(stderr, "unknown switch %s\n", w.c_str());
                return 2;
            }
        }
        const KernelChoice k = select_kernel((Route)route, c, sw, has_image != 0);
        const Kernel at = pick_kernel(k, batch, cus, sw);
        auto name = [](Kernel q) {  // tblock64_kernel's two forms share the function name
            return q == K_NONE ? "none" : q == K_TBLOCK64_TILES ? "tblock64_kernel:tiles" : kernel_name(q);
        };
        printf("%s %s %s %ld\n", name(k.small), name(k.stream), name(at), conv_image_elems(at, c));
    }
    return 0;
}
