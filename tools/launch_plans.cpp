// launch_plans.cpp -- every launch plan of libmifsk.so without a device: the planner of
// minimodem_amd/csrc/mifsk_plan.cpp (plan_launch) over every bit length 3..320 at three rates,
// the named modes, the 187 frame shapes of tests/_shapes.py (1 .. 64 bit windows a frame) at six
// rates, eight batch sizes, three row lengths and every variant of a call, one line per case with
// every field of the plan, and the invariants of a plan checked on each.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc
//       -fsanitize=address,undefined -o launch_plans tools/launch_plans.cpp
//       minimodem_amd/csrc/mifsk_plan.cpp minimodem_amd/csrc/mifsk_config.cpp && ./launch_plans
//
//   launch_plans [--ncu N]                    the fixture (tests/golden/launch_plans.txt): one digest line
//                                             per configuration over its cases' lines; for the named modes,
//                                             plain and under MIFSK_CHAIN=2,3, each distinct plan in full too
//   launch_plans [--ncu N] --full             every line in full
//   launch_plans [--ncu N] --named            the named modes' lines in full (no forced-chain leg)
//   launch_plans [--ncu N] --only LABEL       one configuration's lines (LABEL as in its digest line)
//   launch_plans [--ncu N] --one MODE NSTREAMS NSAMPLES VARIANT FORCE     one case
//
// A frame shape's LABEL / MODE is RATE/SHAPE: 240/raw43 (--binary-raw 43 at 240 baud), 1200/7-13-1.5
// (7 data bits, 13 start bits, 1.5 stop bits), b40.4/8-1-1 (40.4 samples per bit at 48 kHz).
//
// The summary goes to stderr: "launch_plans: N cases, M distinct plans, K chained, 0 violations";
// exit status 1 with a violation.  (tests/test_launch_plans.py)
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "mifsk.h"
#include "mifsk_device.h"

using namespace mifsk;

static const char *const kNamed[] = { "1200", "300", "rtty", "tdd", "same", "12000", "2400", "uic-train",
				      "uic-ground", "callerid", "V.21", "50" };
static const int kStreams[] = { 1, 5, 256, 1024, 3000, 4096, 8192, 65536 };
static const uint32_t kSamples[] = { 0u, 96000u, 1440000u };
static const char *const kVariants[] = { "plain", "ring", "auto", "state", "counters" };
static const char *const kForces[] = { "lib", "wave", "workgroup" };
static const double kDeltas[] = { 0.0, -0.3, 0.4 };
// the frame-shape leg's rates (tests/_shapes.py): a baud rate, or the samples per bit at 48 kHz
static const struct { const char *label; double baud, spb; } kShapeRates[] = {
    { "1200", 1200.0, 0.0 }, { "b40.4", 0.0, 40.4 }, { "12000", 12000.0, 0.0 },
    { "240", 240.0, 0.0 }, { "b300.4", 0.0, 300.4 }, { "45.45", 45.45, 0.0 } };
static const int kShapeData[] = { 5, 7, 8 };
static const int kShapeStart[] = { 0, 1, 2, 3, 7, 13, 20 };
static const float kShapeStop[] = { 0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f };

// a frame shape: --binary-raw N, or data bits - start bits - stop bits
struct Shape {
    int		raw, n_data, nstart;
    float	nstop;
};

static int g_ncu = 256;
static long g_cases = 0, g_chained = 0, g_violations = 0;
static std::set<std::string> g_distinct;

struct Config {
    std::string		label;
    mifsk_rx_config	cfg, cfg_auto;	// (--auto-carrier is an option of the configuration)
    DevCfg		d, d_auto;
};

static std::string shape_label( const Shape &s )
{
    char b[48];
    if ( s.raw )
	std::snprintf(b, sizeof(b), "raw%d", s.raw);
    else
	std::snprintf(b, sizeof(b), "%d-%d-%g", s.n_data, s.nstart, (double)s.nstop);
    return b;
}

// "RATE/SHAPE" -> the rate's baudmode string and the shape; false: not such a label
static bool parse_shape_label( const char *label, std::string &mode, Shape &s )
{
    const char *slash = std::strchr(label, '/');
    if ( !slash )
	return false;
    const std::string rate(label, slash);
    mode.clear();
    for ( const auto &r : kShapeRates )
	if ( rate == r.label ) {
	    char b[64];
	    if ( r.spb != 0.0 )
		std::snprintf(b, sizeof(b), "%.17g", 48000.0 / r.spb);
	    else
		std::snprintf(b, sizeof(b), "%s", r.label);
	    mode = b;
	}
    s = Shape{0, 0, 0, 0.0f};
    if ( mode.empty() )
	return false;
    if ( std::sscanf(slash + 1, "raw%d", &s.raw) == 1 )
	return s.raw > 0 && shape_label(s) == slash + 1;
    return std::sscanf(slash + 1, "%d-%d-%f", &s.n_data, &s.nstart, &s.nstop) == 3 && shape_label(s) == slash + 1;
}

static bool make_config( Config &c, const char *label, const char *mode, const Shape *shape = nullptr )
{
    mifsk_modem_args a;
    mifsk_modem_args_default(&a);
    a.baudmode = mode;
    if ( shape && shape->raw )
	a.binary_raw_nbits = shape->raw;
    else if ( shape ) {
	a.n_data_bits = shape->n_data;
	a.nstartbits = shape->nstart;
	a.nstopbits = shape->nstop;
    }
    if ( mifsk_rx_config_init(&c.cfg, &a) )
	return false;
    a.auto_carrier_threshold = 0.001f;
    if ( mifsk_rx_config_init(&c.cfg_auto, &a) )
	return false;
    fill_devcfg(c.d, c.cfg);
    fill_devcfg(c.d_auto, c.cfg_auto);
    c.label = label;
    return true;
}

#define INVARIANT(cond)	do { if ( !( cond ) ) { g_violations++; \
	std::fprintf(stderr, "VIOLATION %s: %s\n", #cond, line); } } while (0)

static void check( const PlanInputs &in, const LaunchPlan &p, const char *line )
{
    const DevCfg &d = *in.cfg;
    const bool true_kernel = std::strstr(p.kernel_name, ", true>") != nullptr;
    INVARIANT(p.lds_bytes != 0u && p.lds_bytes <= 160u * 1024u);
    INVARIANT(p.chain_groups <= 3u && p.chain_groups <= (uint32_t)in.nstreams);
    INVARIANT(p.chain_groups ? p.chain_chunks >= 2u : p.chain_chunks == 0u);
    INVARIANT(!( p.chain_groups || in.has_state ) || ( true_kernel && p.resumable ));
    INVARIANT(p.resumable == true_kernel);
    INVARIANT(!p.chain_groups || !( in.has_state || in.ring_exact || in.has_counters ));
    INVARIANT(p.frames_per_block <= 64u);
    INVARIANT(p.lattice_mode <= (uint32_t)LAT_DIRECT);
    // what a SCAN slab holds at least: the planner's search reach (+ 8 for the chunked correlator) and 4, in whole float4
    const uint32_t reach = ( ( d.try_max[0] > d.try_max[1] ? d.try_max[0] : d.try_max[1] ) + d.last_reach + 8u + 4u + 3u ) & ~3u;
    if ( p.engine == MIFSK_IO_ENGINE_WAVE ) {
	const WaveGeom &g = p.wave.g;
	INVARIANT(p.workgroup_size == 64u && ( p.wave.sv == 10 || p.wave.sv == 4 ));
	INVARIANT(g.mags_cap % 2u == 0u && g.mags_cap >= 16u * d.n_bits);
	INVARIANT(g.lat_fmin <= g.lat_fmax && g.lat_fmax <= 64u);
	INVARIANT(g.lat_mode != (uint32_t)LAT_LINEAR || ( g.round_wins != 0u && g.round_wins % 64u == 0u ));
	// The tile serves any bit length of at least one step: corr_global_tiled takes whole steps of TILE_K
	// samples, then whole groups of 16, then the tail, whatever B is, and the shared segments are planned
	// per configuration (none below kTileMinBit).  kTileMinBit is where the planner PREFERS the tile to a
	// slab; below it the tile is what is left when no SCAN slab fits a wave's share of LDS -- 200 samples
	// per bit with 43 and more windows a frame, 160 with 52 and more -- and tests/test_gpu_frameshapes.py
	// runs those plans against the oracle (240 baud, --binary-raw 43 .. 64).
	INVARIANT(!g.tiled || ( d.bit_nsamples >= TILE_K && !in.ring_exact ));
	INVARIANT(g.slab_cap == 0u || g.slab_cap >= reach);
	// (the kernel's LDS: counters, magnitudes, slab)
	INVARIANT(p.lds_bytes >= kCntBytes + g.mags_cap * 8u + g.slab_floats * 4u);
    } else {
	const auto &g = p.wg;
	const uint32_t wins = d.lat_grid ? g.lat_frames * ( d.n_bits - 1u ) + 1u : g.lat_frames * d.n_bits;
	INVARIANT(p.engine == MIFSK_IO_ENGINE_WORKGROUP && p.workgroup_size == 64u * ( g.nworkers + 1u ));
	INVARIANT(!in.ring_exact && !in.autodetect);
	INVARIANT(g.lat_frames * g.lat_rounds <= (uint32_t)P_CAP);
	INVARIANT(g.lat_frames == 0u || wins * g.lat_rounds <= (uint32_t)W_CAP);
	INVARIANT(g.lat_mode != (uint32_t)LAT_LINEAR || g.region_cap <= 64u * STAGE_VEC * 4u);
	INVARIANT(g.use_slab || ( g.slab_cap == 0u && g.lat_frames == 0u && g.lat_mode == (uint32_t)LAT_NONE ));
	INVARIANT(g.slab_cap == 0u || g.slab_cap >= reach);
    }
}

// one case: its line into `out` (false: the variant does not take this engine)
static bool one_case( const Config &c, int nstreams, uint32_t nsamples, int variant, int force, std::string &out )
{
    if ( force == 2 && ( variant == 1 || variant == 2 ) )
	return false;		// (the workgroup engine has neither RING addressing nor --auto-carrier)
    PlanInputs in = {};
    in.cfg = variant == 2 ? &c.d_auto : &c.d;
    in.ncu = g_ncu;
    in.nstreams = nstreams;
    in.nsamples = nsamples;
    in.samplebuf_size = ( variant == 2 ? c.cfg_auto : c.cfg ).samplebuf_size;
    in.engine_flags = force == 1 ? MIFSK_IO_ENGINE_WAVE : force == 2 ? MIFSK_IO_ENGINE_WORKGROUP : 0u;
    in.ring_exact = variant == 1;
    in.autodetect = variant == 2;
    in.has_state = variant == 3;
    in.has_counters = variant == 4;
    LaunchPlan p;
    const int rc = plan_launch(in, p);
    char line[512];
    int n = std::snprintf(line, sizeof(line), "%s n=%d ns=%u %s/%s : rc=%d", c.label.c_str(), nstreams, nsamples,
			  kVariants[variant], kForces[force], rc);
    if ( rc == 0 ) {
	n += std::snprintf(line + n, sizeof(line) - (size_t)n, " engine=%s k=%u wps=%u wg=%u lds=%u lat=%u fpb=%u st=%d chain=%ux%u",
			   p.engine == MIFSK_IO_ENGINE_WAVE ? "wave" : "workgroup", p.kernel, p.waves_per_simd,
			   p.workgroup_size, p.lds_bytes, p.lattice_mode, p.frames_per_block, p.resumable ? 1 : 0,
			   p.chain_groups, p.chain_chunks);
	if ( p.engine == MIFSK_IO_ENGINE_WAVE ) {
	    const WaveGeom &g = p.wave.g;
	    n += std::snprintf(line + n, sizeof(line) - (size_t)n, " geom=%u,%u,%u,%u,%u,%u,%u,%u,%d", g.mags_cap, g.slab_floats,
			       g.slab_cap, g.tiled, g.lat_mode, g.lat_fmax, g.lat_fmin, g.round_wins, p.wave.sv);
	} else {
	    const auto &g = p.wg;
	    n += std::snprintf(line + n, sizeof(line) - (size_t)n, " geom=%u,%d,%u,%u,%u,%u,%u,%u", g.nworkers, g.use_slab ? 1 : 0,
			       g.slab_cap, g.lat_frames, g.lat_rounds, g.region_floats, g.region_cap, g.lat_mode);
	}
	std::snprintf(line + n, sizeof(line) - (size_t)n, " kernel=%s", p.kernel_name);
	check(in, p, line);
	g_chained += p.chain_groups != 0u;
    } else {
	g_violations++;
	std::fprintf(stderr, "VIOLATION no plan: %s\n", line);
    }
    g_cases++;
    g_distinct.insert(std::strstr(line, " : "));
    out = line;
    return true;
}

// every case of a configuration: printed in full, or as one FNV-1a digest line over those lines --
// with `plans`, followed by each distinct plan once, in full, in the order of its first case
static void all_cases( const Config &c, bool full, bool plans = false )
{
    uint64_t h = 0xcbf29ce484222325ull;
    long lines = 0;
    std::string line;
    std::vector<std::string> distinct;
    for ( int n : kStreams )
	for ( uint32_t ns : kSamples )
	    for ( int v = 0; v < 5; v++ )
		for ( int f = 0; f < 3; f++ ) {
		    if ( !one_case(c, n, ns, v, f, line) )
			continue;
		    lines++;
		    if ( full )
			std::printf("%s\n", line.c_str());
		    const std::string plan = line.substr(line.find(" : ") + 3);
		    if ( std::find(distinct.begin(), distinct.end(), plan) == distinct.end() )
			distinct.push_back(plan);
		    for ( const char *q = line.c_str(); ; q++ ) {
			h = ( h ^ (unsigned char)( *q ? *q : '\n' ) ) * 0x100000001b3ull;
			if ( !*q )
			    break;
		    }
		}
    if ( full )
	return;
    std::printf("%s digest=%016" PRIx64 " lines=%ld\n", c.label.c_str(), h, lines);
    for ( size_t i = 0; plans && i < distinct.size(); i++ )
	std::printf("%s plan %zu : %s\n", c.label.c_str(), i, distinct[i].c_str());
}

int main( int argc, char **argv )
{
    bool full = false, named_only = false;
    const char *only = nullptr;
    char **one = nullptr;
    for ( int i = 1; i < argc; i++ ) {
	if ( !std::strcmp(argv[i], "--ncu") && i + 1 < argc )
	    g_ncu = std::atoi(argv[++i]);
	else if ( !std::strcmp(argv[i], "--full") )
	    full = true;
	else if ( !std::strcmp(argv[i], "--named") )
	    named_only = true;
	else if ( !std::strcmp(argv[i], "--only") && i + 1 < argc )
	    only = argv[++i];
	else if ( !std::strcmp(argv[i], "--one") && i + 5 < argc ) {
	    one = argv + i + 1;
	    i += 5;
	} else {
	    std::fprintf(stderr, "usage: launch_plans [--ncu N] [--full | --named | --only LABEL | --one MODE NSTREAMS NSAMPLES VARIANT FORCE]\n");
	    return 2;
	}
    }
    // (the knobs are the planner's inputs too: none but the forced-chain leg's below)
    unsetenv("MIFSK_EXPERIMENT");
    static Config c;
    if ( one ) {
	int v = -1, f = -1;
	for ( int k = 0; k < 5; k++ ) if ( !std::strcmp(one[3], kVariants[k]) ) v = k;
	for ( int k = 0; k < 3; k++ ) if ( !std::strcmp(one[4], kForces[k]) ) f = k;
	std::string line;
	std::string mode = one[0];
	Shape shape;
	const bool shaped = parse_shape_label(one[0], mode, shape);
	if ( v < 0 || f < 0 || !make_config(c, one[0], mode.c_str(), shaped ? &shape : nullptr)
		|| !one_case(c, std::atoi(one[1]), (uint32_t)std::strtoul(one[2], nullptr, 10), v, f, line) )
	    return 2;
	std::printf("%s\n", line.c_str());
	return g_violations ? 1 : 0;
    }
    // a configuration's cases, unless another one is asked for; false: mifsk_rx_config_init refuses it
    auto visit = [&]( const std::string &label, const char *mode, bool in_full, bool plans, const Shape *shape = nullptr ) -> bool {
	if ( only && label != only )
	    return true;
	if ( !make_config(c, label.c_str(), mode, shape) )
	    return false;
	all_cases(c, in_full || only, plans);
	return true;
    };
    for ( const char *mode : kNamed )
	if ( !visit(mode, mode, full || named_only, true) )
	    return 2;
    if ( !named_only ) {
	// the forced-chain leg: what MIFSK_CHAIN cuts, and what it must leave alone
	setenv("MIFSK_EXPERIMENT", "1", 1);
	setenv("MIFSK_CHAIN", "2,3", 1);
	for ( const char *mode : kNamed )
	    if ( !visit(std::string("chain2,3:") + mode, mode, full, true) )
		return 2;
	unsetenv("MIFSK_EXPERIMENT");
	unsetenv("MIFSK_CHAIN");
    }
    long refused = 0;
    for ( int B = 3; B <= 320 && !named_only; B++ )
	for ( double dl : kDeltas ) {
	    char label[32], mode[64];
	    std::snprintf(label, sizeof(label), "B%d%+.1f", B, dl);
	    std::snprintf(mode, sizeof(mode), "%.17g", 48000.0 / ( B + dl ));
	    if ( !visit(label, mode, full, false) )
		refused++;		// ((3, 2.7) and nothing else)
	    else if ( ( !only || label == std::string(only) ) && c.cfg.bit_nsamples != (unsigned)B ) {
		g_violations++;
		std::fprintf(stderr, "VIOLATION %s: bit_nsamples %u\n", label, c.cfg.bit_nsamples);
	    }
	}
    if ( !named_only && !only && refused != 1 ) {
	g_violations++;
	std::fprintf(stderr, "VIOLATION %ld configurations refused\n", refused);
    }
    // the frame-shape leg: every number of bit windows a frame may have, at the six rates
    if ( !named_only ) {
	std::vector<Shape> shapes;
	for ( int n = 1; n <= 64; n++ )
	    shapes.push_back(Shape{n, 0, 0, 0.0f});
	for ( int nd : kShapeData )
	    for ( int st : kShapeStart )
		for ( float sp : kShapeStop )
		    if ( !( st == 0 && sp == 3.0f ) )
			shapes.push_back(Shape{0, nd, st, sp});
	for ( const auto &r : kShapeRates )
	    for ( const Shape &sh : shapes ) {
		const std::string label = std::string(r.label) + "/" + shape_label(sh);
		std::string mode;
		Shape parsed;
		if ( !parse_shape_label(label.c_str(), mode, parsed) || !visit(label, mode.c_str(), full, false, &sh) ) {
		    g_violations++;
		    std::fprintf(stderr, "VIOLATION %s: refused\n", label.c_str());
		}
	    }
    }
    std::fprintf(stderr, "launch_plans: %ld cases, %zu distinct plans, %ld chained, %ld violations\n",
		 g_cases, g_distinct.size(), g_chained, g_violations);
    return g_violations ? 1 : 0;
}
