/* readsb_gpu_ifile — `readsb --device-type ifile --ifile X --iformat F --raw --mlat [--stats]`
 * with the demodulator on the GPU: prints one `@<12-hex 12 MHz timestamp><frame hex>;` line per
 * accepted message exactly as displayModesMessage does in --raw --mlat mode (mode_s.c:1834-1847),
 * and with --stats the demodulator counters of display_stats (stats.c:65-125).
 * --sbs-out PATH: instead of the raw lines, the BaseStation feed of the capture (modesSendSBSOutput, net_io.c:3184-3404) into PATH,
 * with nothing but the text leaving the GPU: feed -> field decode -> tracking gate -> position decode -> SBS encoder (sbs_gpu.c).
 * --asterix-out PATH: the same chain ending in the ASTERIX CAT021 encoder (modesSendAsterixOutput, net_io.c:2416-2945).
 * --dump-out PATH: the decoded-message dump of the capture — what the reference prints to stdout without --quiet (displayModesMessage,
 * mode_s.c:1809-2239) — into PATH by the resident chain feed -> field decode -> dump encoder (dump_gpu.c).
 * --snip LEVEL: `readsb --snip <level>` (snipMode, readsb.c:1187-1206) instead of demodulating: stdin (or --ifile) to stdout (snip_gpu.c).
 */
#include <fcntl.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <unistd.h>

#include <time.h>

#include "readsb_gpu_host.h"

static void print_raw_line(FILE *out, const struct gpu_modes_message *mm) {
    static const char hexl[] = "0123456789abcdef", hexu[] = "0123456789ABCDEF";
    char line[1 + 12 + 28 + 2], *p = line;
    *p++ = '@';
    for (int sh = 44; sh >= 0; sh -= 4) *p++ = hexu[((uint64_t) mm->timestamp >> sh) & 15];     /* %012 PRIX64 */
    for (int j = 0; j < mm->msgbits / 8; j++) { *p++ = hexl[mm->msg[j] >> 4]; *p++ = hexl[mm->msg[j] & 15]; }
    *p++ = ';'; *p++ = '\n';
    fwrite(line, 1, (size_t) (p - line), out);
}

static void print_raw(const struct gpu_modes_message *mm, void *user) { print_raw_line(user, mm); }

static const char usage[] =
    "readsb_gpu_ifile --ifile PATH|- [--iformat UC8|SC16|SC16Q11] [--fix|--no-fix|--aggressive] [--no-fix-df] [--modeac]\n"
    "                 [--preamble-threshold N] [--gpu-device N] [--gpu-chunk-buffers N] [--startup-time-ms MS] [--stats] [--raw --mlat]\n"
    "                 [--sbs-out PATH [--sbs-now-ms MS] [--lat DEG --lon DEG] [--gnss]]\n"
    "                 [--asterix-out PATH [--asterix-now-ms MS] [--lat DEG --lon DEG]]\n"
    "                 [--dump-out PATH [--raw] [--mlat] [--dump-onlyaddr] [--show-only HEX]]\n"
    "readsb_gpu_ifile --snip LEVEL [--ifile PATH|-] [--gpu-device N]\n"
    "  default: one `@<timestamp><frame>;` line per accepted message on stdout (readsb --raw --mlat)\n"
    "  --sbs-out PATH   write the BaseStation (port 30003) lines of the capture to PATH instead; the messages, their field records,\n"
    "                   the tracking gate's verdicts and the decoded positions stay on the GPU, only the text comes back.\n"
    "                   Messages whose forwarding is the position tracker's decision (deferred by the gate) are DROPPED, as\n"
    "                   readsb_gpu_gather --forward-only drops them; their number is reported on stderr.  Not with --modeac.\n"
    "  --sbs-now-ms MS  the time printed in fields 9 and 10 (ms since 1970; default: the clock when the program starts)\n"
    "  --asterix-out PATH  write the ASTERIX CAT021 target reports of the capture (the asterix_out connector's stream) to PATH instead,\n"
    "                   by the same resident chain; deferred messages are DROPPED likewise.  No receiver ids, fresh aircraft state.\n"
    "  --asterix-now-ms MS  the clock of I021/077 and of the day's midnight (ms since 1970; default: the clock when the program starts)\n"
    "  --dump-out PATH  write the decoded-message dump of every message (what readsb prints to stdout without --quiet) to PATH instead,\n"
    "                   formatted on the GPU; --raw, --mlat and --dump-onlyaddr select readsb's modes of that output (only here: the\n"
    "                   default output stays the --raw --mlat line), --show-only HEX keeps the messages of one address.  No tracker\n"
    "                   runs, so the file equals the reference program's stdout EXCEPT that `reduce_forward:` always prints 0 and\n"
    "                   every CPR block has the `CPR decoding:  none` form (no decoded position, NIC or Rc lines).  Not with --modeac.\n"
    "  --lat, --lon     the receiver's location (enables positions relative to the receiver and surface positions)\n"
    "  --gnss           Modes.use_gnss: geometric altitudes and rates with the H suffix where available\n"
    "  --snip LEVEL     readsb --snip: copy UC8 samples from stdin (or --ifile PATH) to stdout, every stretch of samples with\n"
    "                   |I - 127| < LEVEL and |Q - 127| < LEVEL cut down to its first 32; nothing is demodulated\n";

/* readsb_amd/host/sbs_gpu.c; absent from builds against a stand-in library, which have no device to keep anything on */
#pragma weak gpu_sbs_run
/* readsb_amd/host/dump_gpu.c; absent likewise */
#pragma weak gpu_dump_run
/* readsb_amd/host/snip_gpu.c; absent likewise (a stand-in library has no mgpu_snip) */
#pragma weak gpu_snip_run

int main(int argc, char **argv) {
    struct mgpu_config cfg;
    mgpu_config_defaults(&cfg);
    const char *ifile = NULL;
    input_format_t fmt = INPUT_UC8;
    int stats = 0;
    unsigned chunk = 256;
    struct gpu_sbs_opts sbs = {NULL, -1, 0, 0, 0.0, 0.0, 0};
    struct gpu_dump_opts dump = {NULL, 0, 0};
    int have_lat = 0, have_lon = 0, snip = 0, snip_level = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--ifile") && i + 1 < argc) ifile = argv[++i];
        else if (!strcmp(argv[i], "--iformat") && i + 1 < argc) {
            const char *f = argv[++i];
            fmt = !strcasecmp(f, "UC8") ? INPUT_UC8 : !strcasecmp(f, "SC16") ? INPUT_SC16 : INPUT_SC16Q11;
        } else if (!strcmp(argv[i], "--fix")) cfg.nfix_crc = 1;
        else if (!strcmp(argv[i], "--no-fix")) cfg.nfix_crc = 0;
        else if (!strcmp(argv[i], "--aggressive")) cfg.nfix_crc = 2;
        else if (!strcmp(argv[i], "--no-fix-df")) cfg.fixDF = 0;
        else if (!strcmp(argv[i], "--modeac")) cfg.mode_ac = 1;        /* Modes.mode_ac, readsb.c:1479 */
        else if (!strcmp(argv[i], "--preamble-threshold") && i + 1 < argc) cfg.preamble_threshold = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gpu-device") && i + 1 < argc) cfg.device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gpu-chunk-buffers") && i + 1 < argc) chunk = (unsigned) atoi(argv[++i]);
        else if (!strcmp(argv[i], "--startup-time-ms") && i + 1 < argc) cfg.startup_time_ms = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--stats")) stats = 1;
        else if (!strcmp(argv[i], "--sbs-out") && i + 1 < argc) { sbs.path = argv[++i]; sbs.asterix = 0; }
        else if (!strcmp(argv[i], "--asterix-out") && i + 1 < argc) { sbs.path = argv[++i]; sbs.asterix = 1; }
        else if ((!strcmp(argv[i], "--sbs-now-ms") || !strcmp(argv[i], "--asterix-now-ms")) && i + 1 < argc) sbs.now_ms = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--lat") && i + 1 < argc) { sbs.lat = atof(argv[++i]); have_lat = 1; }
        else if (!strcmp(argv[i], "--lon") && i + 1 < argc) { sbs.lon = atof(argv[++i]); have_lon = 1; }
        else if (!strcmp(argv[i], "--gnss")) sbs.gnss = 1;
        else if (!strcmp(argv[i], "--snip") && i + 1 < argc) { snip = 1; snip_level = atoi(argv[++i]); }     /* readsb.c:1581-1583 */
        else if (!strcmp(argv[i], "--help")) { fputs(usage, stdout); return 0; }
        else if (!strcmp(argv[i], "--dump-out") && i + 1 < argc) dump.path = argv[++i];
        else if (!strcmp(argv[i], "--dump-onlyaddr")) dump.flags |= MGPU_DUMP_ONLYADDR;
        else if (!strcmp(argv[i], "--show-only") && i + 1 < argc) { dump.show_only = (uint32_t) strtoul(argv[++i], NULL, 16); dump.flags |= MGPU_DUMP_QUIET; }
        else if (!strcmp(argv[i], "--raw")) dump.flags |= MGPU_DUMP_RAW;          /* (read with --dump-out only) */
        else if (!strcmp(argv[i], "--mlat")) dump.flags |= MGPU_DUMP_MLAT;
        else if (!strcmp(argv[i], "--quiet")) { }
        else if (!strcmp(argv[i], "--device-type") && i + 1 < argc) ++i;
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (snip) {
        if (!gpu_snip_run) { fprintf(stderr, "--snip: this build has no GPU chain\n"); return 2; }
        int sfd = !ifile || !strcmp(ifile, "-") ? STDIN_FILENO : open(ifile, O_RDONLY);
        if (sfd < 0) { perror(ifile); return 1; }
        int src = gpu_snip_run(&cfg, sfd, snip_level);
        if (sfd != STDIN_FILENO) close(sfd);
        return src == MGPU_OK ? 0 : 1;
    }
    sbs.have_ref = have_lat && have_lon;
    if (sbs.path && !gpu_sbs_run) { fprintf(stderr, "--sbs-out / --asterix-out: this build has no GPU chain\n"); return 2; }
    if (sbs.path && cfg.mode_ac) { fprintf(stderr, "--sbs-out / --asterix-out: not with --modeac (its replies are merged on the host)\n"); return 2; }
    if (dump.path && !gpu_dump_run) { fprintf(stderr, "--dump-out: this build has no GPU chain\n"); return 2; }
    if (dump.path && (cfg.mode_ac || sbs.path)) { fprintf(stderr, "--dump-out: not with --modeac, --sbs-out or --asterix-out\n"); return 2; }
    if (sbs.path && sbs.now_ms < 0) {
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        sbs.now_ms = (int64_t) ts.tv_sec * 1000 + ts.tv_nsec / 1000000;
    }
    if (!ifile) { fprintf(stderr, "SDR type 'ifile' requires an --ifile argument\n"); return 2; }   /* sdr_ifile.c:118 */
    int fd = !strcmp(ifile, "-") ? STDIN_FILENO : open(ifile, O_RDONLY);
    if (fd < 0) { perror(ifile); return 1; }
    cfg.format = (int) fmt;
    cfg.max_samples = (uint64_t) chunk * 131072;
    struct gpu_demod g;
    if (gpu_demod_open(&g, &cfg, print_raw, stdout) != MGPU_OK) return 1;
    int rc = dump.path ? gpu_dump_run(g.ctx, fd, fmt, chunk, &dump, &g.counters)
             : sbs.path ? gpu_sbs_run(g.ctx, fd, fmt, chunk, &sbs, &g.counters) : gpu_ifile_run(&g, fd, fmt, chunk);
    if (rc != MGPU_OK && !sbs.path && !dump.path) fprintf(stderr, "gpu_ifile_run: %s (%s)\n", mgpu_strerror(rc), mgpu_last_error(g.ctx));
    fflush(stdout);
    if (stats && rc == MGPU_OK) {
        const struct mgpu_counters *c = &g.counters;
        fprintf(stderr, "Local receiver:\n  %" PRIu64 " samples processed\n  %" PRIu64 " samples lost\n", c->samples_processed, c->samples_lost);
        fprintf(stderr, "  %" PRIu64 " Mode-S message preambles received\n", c->demod_preambles);
        fprintf(stderr, "    %" PRIu64 " with bad message format or invalid CRC\n", c->demod_rejected_bad);
        fprintf(stderr, "    %" PRIu64 " with unrecognized ICAO address\n", c->demod_rejected_unknown_icao);
        fprintf(stderr, "    %" PRIu64 " accepted with correct CRC\n", c->demod_accepted[0]);
        for (int i = 1; i <= 2; i++) fprintf(stderr, "    %" PRIu64 " accepted with %d-bit error repaired\n", c->demod_accepted[i], i);
        fprintf(stderr, "  %" PRIu64 " strong signals (> -3dBFS)\n", c->strong_signal_count);
    }
    gpu_demod_close(&g);
    if (fd != STDIN_FILENO) close(fd);
    return rc == MGPU_OK ? 0 : 1;
}
