// mifsk_tables.h -- the context's device tables as values: what is uploaded, byte for byte, made
// in plain C++ (mifsk_tables.cpp; tools/ctx_tables_check.cpp compares every double with the oracle's).
#pragma once

#include <cstdint>
#include <vector>

struct TwKey {
    unsigned fftsize, b_mark, b_space, bit_nsamples;
    bool operator==( const TwKey &o ) const
    {
	return fftsize == o.fftsize && b_mark == o.b_mark && b_space == o.b_space
	    && bit_nsamples == o.bit_nsamples;
    }
};

namespace mifsk {

struct DevCfg;

// The bit tables: [max(tw_entries(B), 8)][4] = cos, -sin of the mark band, cos, -sin of the space
// band at sample n < B, 0.0 behind.  Zero-padded: the workgroup kernel consumes the table in chunks
// of 8 (and fetches one half chunk ahead), the wavefront kernel in groups of 16 (one group ahead,
// and keeps groups 0..2 resident): tw_entries()
std::vector<double> bit_table( const TwKey &key );

// cos, -sin of 2 pi k / N for k < N (the spectrum table of fsk_detect_carrier): [N][2]
std::vector<double> spectrum_table( unsigned N );

// Shared segments: every window's rotation factors of scan `kind`, [segment of the window][window],
// `stride` windows a row; empty (stride 0) for a scan without a valid plan.
std::vector<double> rotation_table( const DevCfg &d, int kind, uint32_t &stride );

} // namespace mifsk
