// Device entry points, the weight arena's layout and the tensor loader (wh_model_*).
#include "runtime.h"

namespace
{
	inline int64_t align256( int64_t x ) { return ( x + 255 ) & ~(int64_t)255; }

	Layout makeLayout( const wh_hparams& hp )
	{
		Layout L;
		int64_t o = 0;
		auto take = [ & ]( int64_t bytes ) { const int64_t r = o; o = align256( o + bytes ); return r; };
		const int64_t d = hp.n_audio_state, V = hp.n_vocab;
		L.filters = take( 4ll * hp.n_mels * 201 );
		L.dft = take( 8ll * 800 );
		L.expTab = take( 2ll * EXP_TABLE_ENTRIES );
		L.encPe = take( 4ll * hp.n_audio_ctx * d );
		L.conv1w = take( 2ll * d * conv1Kpad( hp ) );
		L.conv1b = take( 4 * d );
		L.conv2w = take( 2ll * d * 3 * d );
		L.conv2b = take( 4 * d );
		L.lnPostW = take( 4 * d );
		L.lnPostB = take( 4 * d );
		L.enc.resize( hp.n_audio_layer );
		for( auto& e : L.enc )
		{
			e.ln1w = take( 4 * d ); e.ln1b = take( 4 * d );
			e.wqkv = take( 2ll * 3 * d * d ); e.bqkv = take( 4 * 3 * d );
			e.wo = take( 2ll * d * d ); e.bo = take( 4 * d );
			e.ln2w = take( 4 * d ); e.ln2b = take( 4 * d );
			e.w1 = take( 2ll * 4 * d * d ); e.b1 = take( 4 * 4 * d );
			e.w2 = take( 2ll * 4 * d * d ); e.b2 = take( 4 * d );
		}
		L.decPe = take( 4ll * hp.n_text_ctx * d );
		L.te = take( 2ll * V * d );
		L.decLnW = take( 4 * d ); L.decLnB = take( 4 * d );
		L.wcross = take( 2ll * 2 * hp.n_text_layer * d * d );
		L.bcross = take( 4ll * 2 * hp.n_text_layer * d );
		L.dec.resize( hp.n_text_layer );
		for( auto& e : L.dec )
		{
			e.ln1w = take( 4 * d ); e.ln1b = take( 4 * d );
			e.wqkv = take( 2ll * 3 * d * d ); e.bqkv = take( 4 * 3 * d );
			e.wo = take( 2ll * d * d ); e.bo = take( 4 * d );
			e.lncw = take( 4 * d ); e.lncb = take( 4 * d );
			e.wcq = take( 2ll * d * d ); e.bcq = take( 4 * d );
			e.wco = take( 2ll * d * d ); e.bco = take( 4 * d );
			e.ln2w = take( 4 * d ); e.ln2b = take( 4 * d );
			e.w1 = take( 2ll * 4 * d * d ); e.b1 = take( 4 * 4 * d );
			e.w2 = take( 2ll * 4 * d * d ); e.b2 = take( 4 * d );
		}
		L.total = o;
		return L;
	}

	int checkHparams( const wh_hparams* hp )
	{
		if( !hp ) { setError( "hparams is null" ); return WH_E_INVALIDARG; }
		const int d = hp->n_audio_state;
		if( d <= 0 || d != hp->n_text_state || ( d % 64 ) != 0 || hp->n_audio_head * HEAD_DIM != d || hp->n_text_head * HEAD_DIM != d )
		{
			setError( "unsupported model: need n_audio_state == n_text_state == 64 * heads" );
			return WH_E_INVALIDARG;
		}
		if( hp->n_audio_ctx <= 0 || hp->n_audio_ctx > 1536 || hp->n_text_ctx <= 0 || hp->n_text_ctx > 1536 || hp->n_mels <= 0 ||
			3 * hp->n_mels > CONV1_KPAD_MAX || ( hp->n_mels % 8 ) != 0 || hp->n_vocab <= 0 || hp->n_audio_layer <= 0 || hp->n_text_layer <= 0 )
		{
			setError( "unsupported model dimensions" );
			return WH_E_INVALIDARG;
		}
		return 0;
	}

	// the staging buffer of quantized tensors (uploadQuantized): nothing is in flight, every upload waits for its kernel
	void freeStaging( wh_model* m )
	{
		if( m->staging.base ) (void)guardedFree( m->staging );
		m->staging = Allocation{ nullptr, nullptr, 0, nullptr };
	}
}	// namespace

int wh::bindDevice( const wh_model* m )
{
	int cur = -1;
	if( hipGetDevice( &cur ) == hipSuccess && cur == m->device ) return 0;
	WH_HIP( hipSetDevice( m->device ) );
	return 0;
}

// ==================================================================================================================
// device
// ==================================================================================================================
extern "C" {

int wh_device_count( void )
{
	int n = 0;
	if( hipGetDeviceCount( &n ) != hipSuccess ) return 0;
	return n;
}

int wh_device_info( int device, char* name, size_t nameCap, uint64_t* totalMemBytes, int* computeUnits )
{
	hipDeviceProp_t p;
	WH_HIP( hipGetDeviceProperties( &p, device ) );
	if( name && nameCap ) snprintf( name, nameCap, "%s (%s)", p.name, p.gcnArchName );
	if( totalMemBytes ) *totalMemBytes = p.totalGlobalMem;
	if( computeUnits ) *computeUnits = p.multiProcessorCount;
	return 0;
}

int wh_device_set( int device )
{
	WH_HIP( hipSetDevice( device ) );
	return 0;
}

// ==================================================================================================================
// model
// ==================================================================================================================
int64_t wh_model_arena_bytes( const wh_hparams* hp )
{
	if( checkHparams( hp ) ) return -1;
	return makeLayout( *hp ).total;
}

int wh_model_create( const wh_hparams* hp, void* arenaDev, int alreadyFilled, wh_model** out )
{
	if( !out ) { setError( "out is null" ); return WH_E_INVALIDARG; }
	WH_CHECK( checkHparams( hp ) );
	int nDev = 0;
	if( hipGetDeviceCount( &nDev ) != hipSuccess || nDev <= 0 )
	{
		setError( "no HIP device: libwhisper_hip has no CPU fallback" );
		return WH_E_NO_DEVICE;
	}
	wh_model* m = new wh_model();
	m->hp = *hp;
	m->L = makeLayout( *hp );
	if( hipGetDevice( &m->device ) != hipSuccess ) m->device = 0;
	if( arenaDev )
	{
		m->arena = (uint8_t*)arenaDev;
		m->ownsArena = false;
	}
	else
	{
		void* p = nullptr;
		const hipError_t e = hipMalloc( &p, (size_t)m->L.total );
		if( e != hipSuccess ) { delete m; return hipFail( e, "hipMalloc(arena)", __FILE__, __LINE__ ); }
		m->arena = (uint8_t*)p;
		m->ownsArena = true;
	}
	if( alreadyFilled )
		m->finalized = true;
	else
	{
		const hipError_t e = hipMemset( m->arena, 0, (size_t)m->L.total );
		if( e != hipSuccess ) { wh_model_destroy( m ); return hipFail( e, "hipMemset(arena)", __FILE__, __LINE__ ); }
	}
	*out = m;
	return 0;
}

void wh_model_destroy( wh_model* m )
{
	if( !m ) return;
	(void)bindDevice( m );
	freeStaging( m );
	if( m->ownsArena && m->arena ) (void)hipFree( m->arena );
	delete m;
}

static int upload( wh_model* m, int64_t off, const void* src, int64_t bytes )
{
	WH_BIND( m );
	WH_HIP( hipMemcpy( m->arena + off, src, (size_t)bytes, hipMemcpyHostToDevice ) );
	return 0;
}

// ggml tensor types a file may hold (the third int of a tensor record). 0 and 1 are what `isF16` used to say.
enum { GGML_F32 = 0, GGML_F16 = 1 };
static const char* ggmlTypeName( int type )
{
	static const char* const names[] = { "f32", "f16", "q4_0", "q4_1", "q4_2 (removed from ggml)", "q4_3 (removed from ggml)", "q5_0", "q5_1", "q8_0", "q8_1",
		"q2_k", "q3_k", "q4_k", "q5_k", "q6_k", "q8_k" };
	return type >= 0 && type < (int)( sizeof( names ) / sizeof( names[ 0 ] ) ) ? names[ type ] : "unknown";
}

// Quantized blocks of one matrix: host -> the model's staging buffer -> FP16 in the arena (dequant.hip). The staging buffer grows to the largest tensor seen
// and lives until wh_model_finalize or wh_model_destroy; the call returns when the arena holds the values, like upload().
static int uploadQuantized( wh_model* m, int64_t off, int type, const void* src, int64_t nBlocks )
{
	WH_BIND( m );
	const int64_t bytes = nBlocks * dequantBlockBytes( type );
	if( bytes > m->staging.bytes )
	{
		freeStaging( m );
		WH_HIP( guardedAlloc( m->staging, bytes, -1, "quantized tensor staging", nullptr ) );
	}
	WH_HIP( hipMemcpy( m->staging.body, src, (size_t)bytes, hipMemcpyHostToDevice ) );
	WH_CHECK( launchDequantize( nullptr, type, m->staging.body, nBlocks, m->arena + off ) );
	WH_HIP( hipStreamSynchronize( nullptr ) );
	return 0;
}

// Destination of one file tensor. kind: 0 = plain copy, 1 = conv weight (re-ordered), rows x cols is the expected shape.
struct Slot
{
	int64_t off = -1;
	int64_t rows = 0, cols = 0;	   // expected numpy shape (rows, cols); vectors have rows = 1
	bool f16 = false;
	int kind = 0;
	int convIc = 0;
};

static bool parseBlock( const std::string& name, const char* prefix, int& idx, std::string& rest )
{
	const size_t pl = strlen( prefix );
	if( name.compare( 0, pl, prefix ) != 0 ) return false;
	size_t p = pl;
	if( p >= name.size() || !isdigit( (unsigned char)name[ p ] ) ) return false;
	int v = 0;
	while( p < name.size() && isdigit( (unsigned char)name[ p ] ) ) v = v * 10 + ( name[ p++ ] - '0' );
	if( p >= name.size() || name[ p ] != '.' ) return false;
	idx = v;
	rest = name.substr( p + 1 );
	return true;
}

// Tensor name map: Whisper/Whisper/WhisperModel.cpp:63-162 == Whisper/source/whisper.cpp:774-940
static bool resolve( const wh_model* m, const std::string& name, Slot& s )
{
	const wh_hparams& hp = m->hp;
	const Layout& L = m->L;
	const int64_t d = hp.n_audio_state;
	auto mat = [ & ]( int64_t off, int64_t rows, int64_t cols ) { s.off = off; s.rows = rows; s.cols = cols; s.f16 = true; return true; };
	auto vec = [ & ]( int64_t off, int64_t n ) { s.off = off; s.rows = 1; s.cols = n; s.f16 = false; return true; };
	if( name == "encoder.positional_embedding" ) { s.off = L.encPe; s.rows = hp.n_audio_ctx; s.cols = d; s.f16 = false; return true; }
	if( name == "encoder.conv1.weight" ) { s.kind = 1; s.convIc = hp.n_mels; return mat( L.conv1w, d, 3ll * hp.n_mels ); }
	if( name == "encoder.conv1.bias" ) return vec( L.conv1b, d );
	if( name == "encoder.conv2.weight" ) { s.kind = 1; s.convIc = (int)d; return mat( L.conv2w, d, 3 * d ); }
	if( name == "encoder.conv2.bias" ) return vec( L.conv2b, d );
	if( name == "encoder.ln_post.weight" ) return vec( L.lnPostW, d );
	if( name == "encoder.ln_post.bias" ) return vec( L.lnPostB, d );
	if( name == "decoder.positional_embedding" ) { s.off = L.decPe; s.rows = hp.n_text_ctx; s.cols = d; s.f16 = false; return true; }
	if( name == "decoder.token_embedding.weight" ) return mat( L.te, hp.n_vocab, d );
	if( name == "decoder.ln.weight" ) return vec( L.decLnW, d );
	if( name == "decoder.ln.bias" ) return vec( L.decLnB, d );
	int il = 0;
	std::string r;
	if( parseBlock( name, "encoder.blocks.", il, r ) )
	{
		if( il >= hp.n_audio_layer ) return false;
		const EncLayer& e = L.enc[ il ];
		if( r == "attn_ln.weight" ) return vec( e.ln1w, d );
		if( r == "attn_ln.bias" ) return vec( e.ln1b, d );
		if( r == "attn.query.weight" ) return mat( e.wqkv, d, d );
		if( r == "attn.query.bias" ) return vec( e.bqkv, d );
		if( r == "attn.key.weight" ) return mat( e.wqkv + 2 * d * d, d, d );
		if( r == "attn.value.weight" ) return mat( e.wqkv + 4 * d * d, d, d );
		if( r == "attn.value.bias" ) return vec( e.bqkv + 8 * d, d );
		if( r == "attn.out.weight" ) return mat( e.wo, d, d );
		if( r == "attn.out.bias" ) return vec( e.bo, d );
		if( r == "mlp_ln.weight" ) return vec( e.ln2w, d );
		if( r == "mlp_ln.bias" ) return vec( e.ln2b, d );
		if( r == "mlp.0.weight" ) return mat( e.w1, 4 * d, d );
		if( r == "mlp.0.bias" ) return vec( e.b1, 4 * d );
		if( r == "mlp.2.weight" ) return mat( e.w2, d, 4 * d );
		if( r == "mlp.2.bias" ) return vec( e.b2, d );
		return false;
	}
	if( parseBlock( name, "decoder.blocks.", il, r ) )
	{
		if( il >= hp.n_text_layer ) return false;
		const DecLayer& e = L.dec[ il ];
		if( r == "attn_ln.weight" ) return vec( e.ln1w, d );
		if( r == "attn_ln.bias" ) return vec( e.ln1b, d );
		if( r == "attn.query.weight" ) return mat( e.wqkv, d, d );
		if( r == "attn.query.bias" ) return vec( e.bqkv, d );
		if( r == "attn.key.weight" ) return mat( e.wqkv + 2 * d * d, d, d );
		if( r == "attn.value.weight" ) return mat( e.wqkv + 4 * d * d, d, d );
		if( r == "attn.value.bias" ) return vec( e.bqkv + 8 * d, d );
		if( r == "attn.out.weight" ) return mat( e.wo, d, d );
		if( r == "attn.out.bias" ) return vec( e.bo, d );
		if( r == "cross_attn_ln.weight" ) return vec( e.lncw, d );
		if( r == "cross_attn_ln.bias" ) return vec( e.lncb, d );
		if( r == "cross_attn.query.weight" ) return mat( e.wcq, d, d );
		if( r == "cross_attn.query.bias" ) return vec( e.bcq, d );
		if( r == "cross_attn.key.weight" ) return mat( L.wcross + 2 * ( 2ll * il ) * d * d, d, d );
		if( r == "cross_attn.value.weight" ) return mat( L.wcross + 2 * ( 2ll * il + 1 ) * d * d, d, d );
		if( r == "cross_attn.value.bias" ) return vec( L.bcross + 4 * ( 2ll * il + 1 ) * d, d );
		if( r == "cross_attn.out.weight" ) return mat( e.wco, d, d );
		if( r == "cross_attn.out.bias" ) return vec( e.bco, d );
		if( r == "mlp_ln.weight" ) return vec( e.ln2w, d );
		if( r == "mlp_ln.bias" ) return vec( e.ln2b, d );
		if( r == "mlp.0.weight" ) return mat( e.w1, 4 * d, d );
		if( r == "mlp.0.bias" ) return vec( e.b1, 4 * d );
		if( r == "mlp.2.weight" ) return mat( e.w2, d, 4 * d );
		if( r == "mlp.2.bias" ) return vec( e.b2, d );
		return false;
	}
	return false;
}


int wh_model_set_tensor( wh_model* m, const char* name, int nDims, const int32_t* ne, int type, const void* data )
{
	if( !m || !name || !ne || !data || nDims < 1 || nDims > 3 ) { setError( "set_tensor: bad argument" ); return WH_E_INVALIDARG; }
	if( m->finalized ) { setError( "set_tensor: model already finalized" ); return WH_E_INVALIDARG; }
	const bool quantized = dequantBlockBytes( type ) != 0;
	if( type != GGML_F32 && type != GGML_F16 && !quantized )
	{
		setError( std::string( "tensor '" ) + name + "' has ggml type " + std::to_string( type ) + " (" + ggmlTypeName( type ) +
			"): supported are f32, f16, q4_0, q4_1, q5_0, q5_1 and q8_0" );
		return WH_E_INVALIDARG;
	}
	const bool isF16 = type == GGML_F16;
	Slot s;
	if( !resolve( m, name, s ) )
	{
		setError( std::string( "unknown tensor '" ) + name + "' in model file" );
		return WH_E_INVALIDARG;
	}
	if( m->loaded.count( name ) )
	{
		setError( std::string( "tensor '" ) + name + "' appears twice" );
		return WH_E_INVALIDARG;
	}
	int64_t count = 1;
	for( int i = 0; i < nDims; i++ ) count *= ne[ i ];
	if( count != s.rows * s.cols )
	{
		setError( std::string( "tensor '" ) + name + "' has wrong size in model file" );
		return WH_E_INVALIDARG;
	}
	// shape check: ne[0] is the contiguous dimension
	bool shapeOk;
	if( s.kind == 1 )
		shapeOk = nDims == 3 && ne[ 0 ] == 3 && ne[ 1 ] == s.convIc && ne[ 2 ] == s.rows;
	else if( s.rows == 1 )
		shapeOk = ne[ nDims - 1 ] == s.cols || ( nDims >= 1 && ne[ 0 ] == s.cols ) || ( nDims == 2 && ne[ 0 ] == 1 && ne[ 1 ] == s.cols );
	else
		shapeOk = nDims == 2 && ne[ 0 ] == s.cols && ne[ 1 ] == s.rows;
	if( !shapeOk )
	{
		setError( std::string( "tensor '" ) + name + "' has wrong shape in model file" );
		return WH_E_INVALIDARG;
	}

	if( quantized )
	{
		// whisper.cpp's quantizer touches the 2-D *.weight matrices only: the linear layers and the token embedding -- here the plain FP16 matrices of the arena
		if( s.kind != 0 || !s.f16 || s.rows <= 1 )
		{
			setError( std::string( "tensor '" ) + name + "' is stored as " + ggmlTypeName( type ) + ": only the linear layers' weight matrices and the token embedding may be quantized" );
			return WH_E_INVALIDARG;
		}
		if( ( ne[ 0 ] % 32 ) != 0 )
		{
			setError( std::string( "tensor '" ) + name + "' is stored as " + ggmlTypeName( type ) + " but its rows of " + std::to_string( ne[ 0 ] ) + " elements are not whole blocks of 32" );
			return WH_E_INVALIDARG;
		}
		WH_CHECK( uploadQuantized( m, s.off, type, data, count / 32 ) );
	}
	else if( s.kind == 1 )
	{
		// file: [out][in][3] (tap contiguous) -> ours: [out][tap * in + c], row padded with zeros (conv as an implicit GEMM)
		const int64_t ic = s.convIc, oc = s.rows;
		const int64_t kpad = ( s.off == m->L.conv1w ) ? conv1Kpad( m->hp ) : 3 * ic;
		std::vector<uint16_t> tmp( (size_t)( oc * kpad ), 0 );
		for( int64_t o = 0; o < oc; o++ )
			for( int64_t c = 0; c < ic; c++ )
				for( int t = 0; t < 3; t++ )
				{
					const int64_t si = ( o * ic + c ) * 3 + t;
					const uint16_t v = isF16 ? ( (const uint16_t*)data )[ si ] : f32ToF16Bits( ( (const float*)data )[ si ] );
					tmp[ (size_t)( o * kpad + t * ic + c ) ] = v;
				}
		WH_CHECK( upload( m, s.off, tmp.data(), (int64_t)tmp.size() * 2 ) );
	}
	else if( s.f16 )
	{
		if( isF16 )
			WH_CHECK( upload( m, s.off, data, count * 2 ) );
		else
		{
			std::vector<uint16_t> tmp( (size_t)count );
			for( int64_t i = 0; i < count; i++ ) tmp[ (size_t)i ] = f32ToF16Bits( ( (const float*)data )[ i ] );
			WH_CHECK( upload( m, s.off, tmp.data(), count * 2 ) );
		}
	}
	else
	{
		if( !isF16 )
			WH_CHECK( upload( m, s.off, data, count * 4 ) );
		else
		{
			std::vector<float> tmp( (size_t)count );
			for( int64_t i = 0; i < count; i++ ) tmp[ (size_t)i ] = f16BitsToF32( ( (const uint16_t*)data )[ i ] );
			WH_CHECK( upload( m, s.off, tmp.data(), count * 4 ) );
		}
	}
	m->loaded.insert( name );
	return 0;
}

int wh_model_set_filters( wh_model* m, int nMel, int nFft, const float* data )
{
	if( !m || !data ) { setError( "set_filters: bad argument" ); return WH_E_INVALIDARG; }
	if( nMel != m->hp.n_mels || nFft != 201 ) { setError( "mel filterbank must be [n_mels][201]" ); return WH_E_INVALIDARG; }
	WH_CHECK( upload( m, m->L.filters, data, 4ll * nMel * nFft ) );
	m->filtersSet = true;
	return 0;
}

int wh_model_finalize( wh_model* m )
{
	if( !m ) return WH_E_INVALIDARG;
	if( m->finalized ) return 0;
	if( !m->filtersSet )
	{
		// the reference's loader fails on a file without the filterbank (WhisperModel.cpp:446-456); an all-zero one would turn
		// every spectrogram into log10(1e-10) without an error
		setError( "mel filterbank has not been set (wh_model_set_filters)" );
		return WH_E_NOT_READY;
	}
	if( m->loaded.size() != m->expectedTensors() )
	{
		char buf[ 160 ];
		snprintf( buf, sizeof( buf ), "not all tensors loaded from model file - expected %zu, got %zu", m->expectedTensors(), m->loaded.size() );
		setError( buf );
		return WH_E_NOT_READY;
	}
	// DFT twiddles for the mel kernel: cos / sin of 2 pi n / 400 in double (same expression as whisper.cpp:2073-2077)
	std::vector<double> tw( 800 );
	for( int n = 0; n < 400; n++ )
	{
		tw[ n ] = cos( ( 2.0 * M_PI * n ) / 400 );
		tw[ 400 + n ] = sin( ( 2.0 * M_PI * n ) / 400 );
	}
	WH_CHECK( upload( m, m->L.dft, tw.data(), 800 * 8 ) );
	// The reference's exponential IS a table: table_exp_f16[ bits ] = fp16( expf( fp32( fp16 bits ) ) ), built once at start-up
	// (Whisper/source/ggml.c:1375-1385, read at :5069-5080 and :6001-6016). The softmax only ever looks up non-positive arguments, and
	// fp16( expf( x ) ) is 0 below -17.33: entry i here belongs to the FP16 number -|bits i|, i < 0x5000 (entries from 0x4C56 on are 0).
	// Built with the host's expf like the reference builds its own -- all 20480 entries equal the reference's table
	// (tests/test_gpu_ops.py::test_exp_table_in_the_arena). attentionEncT keeps it in LDS: 40 KB next to the K / V tiles.
	{
		std::vector<_Float16> tab( EXP_TABLE_ENTRIES );
		for( uint32_t i = 0; i < (uint32_t)EXP_TABLE_ENTRIES; i++ )
		{
			const uint16_t bits = (uint16_t)( i | 0x8000u );
			_Float16 h;
			memcpy( &h, &bits, 2 );
			tab[ i ] = (_Float16)expf( (float)h );
		}
		WH_CHECK( upload( m, m->L.expTab, tab.data(), EXP_TABLE_ENTRIES * 2 ) );
	}
	freeStaging( m );
	m->finalized = true;
	return 0;
}

int wh_model_arena( wh_model* m, void** dev, int64_t* bytes )
{
	if( !m ) return WH_E_INVALIDARG;
	if( dev ) *dev = m->arena;
	if( bytes ) *bytes = m->L.total;
	return 0;
}

int wh_model_hparams( const wh_model* m, wh_hparams* out )
{
	if( !m || !out ) return WH_E_INVALIDARG;
	*out = m->hp;
	return 0;
}

}	// extern "C"
