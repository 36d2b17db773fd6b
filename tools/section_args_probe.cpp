// The host-side argument checks of launch_track_sections (csrc/sections.hip, through the shared checks of csrc/beat_slots.h), run without
// a GPU: every call below is refused before anything is launched, so this program needs no device.  Meant to be built with the host
// side under sanitizers and run on a CPU-only machine:
//   hipcc --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Iyourmt3_amd/csrc \
//         -Iinclude tools/section_args_probe.cpp yourmt3_amd/csrc/sections.hip -fsanitize=address,undefined -o tools/section_args_probe
//   tools/section_args_probe
// (the second -fsanitize is the link's; the compiler says that it ignores it for the device code, which is what is wanted)
// Exit status 0: every refusal came back with its code.
#include <cstdio>
#include <functional>

#include "kernels.h"

int main() {
    static int32_t beats[4] = {10, 20, 30, 40}, section[4], starts[SECTION_MAX_SECTIONS + 2];
    static long long beat_result[4] = {4, 0, 0, 0}, result[8], nov[4];
    static unsigned chroma[48];
    static unsigned short f[4 * SECTION_F_WORDS];
    static unsigned char peak[4], same[SECTION_MAX_SECTIONS * SECTION_MAX_SECTIONS];
    static unsigned long long acc[SECTION_ACC_WORDS];
    static DetokNote notes[2];
    SectionArgs good{};
    good.frames_per_second = 100.0; good.n_programs = 130; good.drum_program = 128;
    good.near_div = 4; good.context = 1; good.kernel_beats = 4; good.min_len = 8; good.peak_div = 2; good.same_dist = 512; good.len_num = 2; good.max_sections = 32;
    good.beats = beats; good.beat_result = beat_result; good.max_beats = 4; good.notes = notes; good.n = 2; good.n_frames = 100;
    good.chroma = chroma; good.f = f; good.nov = nov; good.peak = peak; good.acc = acc; good.starts = starts; good.same = same;
    good.section = section; good.result = result;
    struct Case { const char* what; int code; std::function<void(SectionArgs&)> change; };
    const Case cases[] = {
        {"n_programs = 0", -1, [](SectionArgs& a) { a.n_programs = 0; }},
        {"n_programs = 257", -1, [](SectionArgs& a) { a.n_programs = 257; }},
        {"drum_program = n_programs", -1, [](SectionArgs& a) { a.drum_program = a.n_programs; }},
        {"context = 0", -2, [](SectionArgs& a) { a.context = 0; }},
        {"context = 17", -2, [](SectionArgs& a) { a.context = 17; }},
        {"kernel_beats = 1", -2, [](SectionArgs& a) { a.kernel_beats = 1; }},
        {"kernel_beats = 65", -2, [](SectionArgs& a) { a.kernel_beats = 65; }},
        {"min_len = 257", -2, [](SectionArgs& a) { a.min_len = 257; }},
        {"max_sections = 0", -2, [](SectionArgs& a) { a.max_sections = 0; }},
        {"max_sections = 65", -2, [](SectionArgs& a) { a.max_sections = 65; }},
        {"peak_div = 0", -3, [](SectionArgs& a) { a.peak_div = 0; }},
        {"same_dist = 32769", -3, [](SectionArgs& a) { a.same_dist = 32769; }},
        {"len_num = 17", -3, [](SectionArgs& a) { a.len_num = 17; }},
        {"near_div = 1", -3, [](SectionArgs& a) { a.near_div = 1; }},
        {"frames_per_second = 0", -3, [](SectionArgs& a) { a.frames_per_second = 0.0; }},
        {"n_frames = 0", -4, [](SectionArgs& a) { a.n_frames = 0; }},
        {"n_frames = 2^20 + 1", -4, [](SectionArgs& a) { a.n_frames = BAR_MAX_FRAMES + 1; }},
        {"n = -1", -4, [](SectionArgs& a) { a.n = -1; }},
        {"n = 2^20 + 1", -4, [](SectionArgs& a) { a.n = BAR_MAX_NOTES + 1; }},
        {"notes NULL with n > 0", -4, [](SectionArgs& a) { a.notes = nullptr; }},
        {"max_beats = 0", -5, [](SectionArgs& a) { a.max_beats = 0; }},
        {"max_beats = 2^20 + 2", -5, [](SectionArgs& a) { a.max_beats = BAR_MAX_BEATS + 1; }},
        {"beats NULL", -6, [](SectionArgs& a) { a.beats = nullptr; }},
        {"beat_result NULL", -6, [](SectionArgs& a) { a.beat_result = nullptr; }},
        {"chroma NULL", -6, [](SectionArgs& a) { a.chroma = nullptr; }},
        {"result NULL", -6, [](SectionArgs& a) { a.result = nullptr; }},
        {"f NULL", -6, [](SectionArgs& a) { a.f = nullptr; }},
        {"nov NULL", -6, [](SectionArgs& a) { a.nov = nullptr; }},
        {"peak NULL", -6, [](SectionArgs& a) { a.peak = nullptr; }},
        {"acc NULL", -6, [](SectionArgs& a) { a.acc = nullptr; }},
        {"starts NULL", -6, [](SectionArgs& a) { a.starts = nullptr; }},
        {"same NULL", -6, [](SectionArgs& a) { a.same = nullptr; }},
        {"section NULL", -6, [](SectionArgs& a) { a.section = nullptr; }},
    };
    int bad = 0;
    for (const Case& c : cases) {
        SectionArgs a = good;
        c.change(a);
        const int rc = launch_track_sections(a, nullptr);
        if (rc != c.code) {
            std::printf("%s: returned %d, expected %d\n", c.what, rc, c.code);
            ++bad;
        }
    }
    std::printf("%d of %d refusals came back with their codes\n", (int)(sizeof cases / sizeof cases[0]) - bad, (int)(sizeof cases / sizeof cases[0]));
    return bad ? 1 : 0;
}
