// The option registry (tuning bits, WH_OPT_* / wh_debug_set_option) and the calling thread's last error.
#include "runtime.h"

namespace wh
{
	unsigned g_tuning = TUNE_DEFAULT;
	Options g_opt;
	namespace
	{
		struct OptionName { const char* name; int Options::* field; };
		const OptionName g_optionNames[] = { { "dec_tile", &Options::decTile }, { "dec_depth", &Options::decDepth }, { "dec_wide_rows", &Options::decWideRows }, { "dec_deep_rows", &Options::decDeepRows }, { "vocab_decrows", &Options::vocabDecRows }, { "enc_chunk", &Options::encChunk },
			{ "self_fuse_max_rows", &Options::selfFuseMaxRows }, { "self_nq", &Options::selfNq }, { "self_wave_min_rows", &Options::selfWaveMinRows }, { "exact_enc_layers", &Options::exactEncLayers }, { "exact_alt_order", &Options::exactAltOrder }, { "enc_exp", &Options::encExp }, { "enc_sched", &Options::encSched }, { "enc_ablate", &Options::encAblate }, { "gemm_mf16", &Options::gemmMf16 }, { "dec_lds", &Options::decLds }, { "dec_lds_ks", &Options::decLdsKs }, { "dec_split", &Options::decSplit }, { "vocab_lds", &Options::vocabLds }, { "beam_regs", &Options::beamRegs }, { "reorder_group", &Options::reorderGroup }, { "gemm_big_min_rows", &Options::gemmBigMinRows }, { "cross_mfma", &Options::crossMfma }, { "resample_lds_phases", &Options::resampleLdsPhases },
			{ "score_chunk_rows", &Options::scoreChunkRows }, { "score_regs", &Options::scoreRegs } };
		// WH_OPT_DEC_TILE=44 ... at load
		const bool g_optionsFromEnv = []()
		{
			for( const OptionName& o : g_optionNames )
			{
				std::string env = "WH_OPT_";
				for( const char* p = o.name; *p; p++ ) env.push_back( (char)toupper( (unsigned char)*p ) );
				if( const char* e = getenv( env.c_str() ) )
				{
					// a number in the options' common range, or the variable is ignored (garbage used to become 0 and re-route kernels silently)
					char* end = nullptr;
					const long v = strtol( e, &end, 10 );
					if( end != e && *end == 0 && v >= -1 && v <= ( 1 << 24 ) ) g_opt.*( o.field ) = (int)v;
					else fprintf( stderr, "[wh] %s='%s' ignored (not an integer in [-1, 2^24])\n", env.c_str(), e );
				}
			}
			return true;
		}();
	}
	static thread_local std::string g_lastError;
	void setError( const std::string& s ) { g_lastError = s; }
	int hipFail( hipError_t e, const char* what, const char* file, int line )
	{
		char buf[ 512 ];
		snprintf( buf, sizeof( buf ), "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString( e ), file, line, what );
		g_lastError = buf;
		return WH_E_HIP;
	}
}

extern "C" {

const char* wh_last_error( void ) { return g_lastError.c_str(); }

int wh_debug_set_tuning( uint32_t mask )
{
	g_tuning = mask;
	return 0;
}

int wh_debug_set_option( const char* name, int value )
{
	if( !name ) { setError( "debug_set_option: null name" ); return WH_E_INVALIDARG; }
	for( const OptionName& o : g_optionNames )
		if( 0 == strcmp( o.name, name ) )
		{
			if( value < -1 || value > ( 1 << 24 ) ) { setError( std::string( "option '" ) + name + "': value out of range" ); return WH_E_INVALIDARG; }
			g_opt.*( o.field ) = value;
			return 0;
		}
	setError( "debug_set_option: unknown option" );
	return WH_E_INVALIDARG;
}

int wh_debug_get_option( const char* name, int* value )
{
	if( !name || !value ) { setError( "debug_get_option: null argument" ); return WH_E_INVALIDARG; }
	for( const OptionName& o : g_optionNames )
		if( 0 == strcmp( o.name, name ) )
		{
			*value = g_opt.*( o.field );
			return 0;
		}
	setError( "debug_get_option: unknown option" );
	return WH_E_INVALIDARG;
}

}	// extern "C"
