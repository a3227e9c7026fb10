// launch_shape_check — the launch geometry on its own: plan.cpp's shape_launch / shape_fast and the three descriptions of a shape, linked with
// plan.cpp and batch_host.cpp only (no kernel unit, no device).  tests/test_launch_shape_cpu.py writes the cases of
// tests/golden/launch_shapes.json (recorded from real launches) as lines of text and runs this program on them:
//   case NAME / params cli|struct MAXLENGTHDEL(-1: the default) / env KEY VALUE / ask <22 scalars> <0|1: a record follows> [17 fields] /
//   last <8 values> / name KERNEL NAME / end
// Every ask is shaped under the case's switches (set in this process' environment, so that read_switches is part of what is checked); its
// dd_launch_log record, and at the end of the case dd_last_launch's eight values and dd_kernel_name's text, must equal the recorded ones
// field by field.  Prints one line per difference and "launch_shape_check: N cases, M asks ok" when there is none.
#include <fstream>
#include <iostream>
#include <sstream>
#include "../dindel_tgi_amd/csrc/capi_internal.h"

using namespace ddh;

static const char *kLogField[DD_LAUNCH_LOG_FIELDS] = {"K", "pairs_per_wave", "D", "gbt", "fold", "waves", "lds_block", "grid", "split", "n_haps", "max_hap",
                                                      "min_read", "max_read", "waves_per_cu", "occ", "us", "dynamic", "reads_per_wave"};
static const char *kLastField[8] = {"K", "D", "waves", "lds_block", "grid", "split", "lds_wave", "lds_shared"};
static int g_failed = 0;

static void differ(const std::string &c, int ask, const char *what, const char *field, long long got, long long want)
{
    std::printf("%s ask %d: %s.%s is %lld, recorded %lld\n", c.c_str(), ask, what, field, got, want);
    g_failed++;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: launch_shape_check CASES.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line, name;
    std::vector<std::string> env;
    dd_params p;
    LaunchShape last;
    int n_cases = 0, n_asks = 0, ask_no = 0;
    while (std::getline(in, line)) {
        std::istringstream is(line);
        std::string key;
        is >> key;
        if (key == "case") {
            is >> name;
            last = LaunchShape();                     // a thread that has launched nothing yet
            ask_no = 0;
        } else if (key == "params") {
            std::string which;
            int mld;
            is >> which >> mld;
            if (which == "struct") dd_params_struct_defaults(&p); else dd_params_cli_defaults(&p);
            if (mld >= 0) p.maxLengthDel = mld;
        } else if (key == "env") {
            std::string k, v;
            is >> k >> v;
            setenv(k.c_str(), v.c_str(), 1);
            env.push_back(k);
        } else if (key == "ask") {
            long long v[22];
            int has_record = 0;
            for (long long &x : v) is >> x;
            is >> has_record;
            if (!is) { std::printf("%s: malformed ask\n", name.c_str()); return 2; }
            LaunchAsk a;
            a.p = &p;
            const bool faster = v[0] != 0;
            a.n_windows = (int)v[1]; a.n_haps = (int)v[2]; a.n_reads = (int)v[3]; a.max_hap_len = (int)v[4]; a.max_read_len = (int)v[5];
            a.n_qual = (int)v[6]; a.max_window_reads = (int)v[7];
            a.has_class = v[8] != 0; a.cls.listed = v[9] != 0; a.cls.list_begin = (int)v[10]; a.cls.list_end = (int)v[11];
            a.cls.max_hap_len = (int)v[12]; a.cls.max_read_len = (int)v[13]; a.cls.min_read_len = (int)v[14];
            a.cls.max_window_reads = (int)v[15]; a.cls.avg_window_reads = (int)v[16]; a.cls.avg_read_len = (int)v[17];
            a.hap_begin = (int)v[18]; a.hap_end = (int)v[19]; a.workspace_bytes = (size_t)v[20]; a.overlapping_chunks = v[21] != 0;
            LaunchShape s;
            ddk::KernelArgs A;
            memset(&A, 0, sizeof(A));
            const Switches sw = read_switches();
            const int rc = faster ? shape_fast(sw, a, s, A) : shape_launch(sw, a, s, A);
            if (rc) { std::printf("%s ask %d: refused (%d: %s)\n", name.c_str(), ask_no, rc, dd_last_error()); g_failed++; }
            else {
                if (s.grid > 0) last = s;
                if (!faster && (s.grid > 0) != (has_record != 0)) differ(name, ask_no, "launch", "launched", s.grid > 0, has_record);
                if (has_record && s.grid > 0) {
                    int32_t got[DD_LAUNCH_LOG_FIELDS];
                    shape_log_record(s, got);
                    for (int i = 0; i < DD_LAUNCH_LOG_FIELDS; i++) {
                        if (i == 15) continue;        // the duration: not part of the shape
                        long long want;
                        is >> want;
                        if (!is) { std::printf("%s: malformed record\n", name.c_str()); return 2; }
                        if (got[i] != want) differ(name, ask_no, "record", kLogField[i], got[i], want);
                    }
                }
            }
            ask_no++;
            n_asks++;
        } else if (key == "last") {
            int32_t got[8];
            shape_last_launch(last, got);
            for (int i = 0; i < 8; i++) {
                long long want;
                is >> want;
                if (got[i] != want) differ(name, -1, "last_launch", kLastField[i], got[i], want);
            }
        } else if (key == "name") {
            std::string want;
            std::getline(is >> std::ws, want);
            char got[64];
            shape_kernel_name(last, got, sizeof(got));
            if (want != got) { std::printf("%s: kernel name is '%s', recorded '%s'\n", name.c_str(), got, want.c_str()); g_failed++; }
        } else if (key == "end") {
            for (const std::string &k : env) unsetenv(k.c_str());
            env.clear();
            n_cases++;
        } else if (!key.empty()) {
            std::printf("unknown line: %s\n", line.c_str());
            return 2;
        }
    }
    {   // a thread that has launched nothing: the main kernel's plain name, eight zeros
        char got[64];
        int32_t v[8];
        shape_kernel_name(LaunchShape(), got, sizeof(got));
        shape_last_launch(LaunchShape(), v);
        if (std::string(got) != "dd_hmm_kernel") { std::printf("no launch: kernel name is '%s'\n", got); g_failed++; }
        for (int i = 0; i < 8; i++)
            if (v[i] != 0) differ("no launch", -1, "last_launch", kLastField[i], v[i], 0);
    }
    if (g_failed) { std::printf("launch_shape_check: %d differences\n", g_failed); return 1; }
    std::printf("launch_shape_check: %d cases, %d asks ok\n", n_cases, n_asks);
    return 0;
}
