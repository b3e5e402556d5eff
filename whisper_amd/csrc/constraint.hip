// Constrained decoding (wh_context_set_constraint; DESIGN.md section 7 "Constrained decoding"): the two kernels and their launches. filters.hip owns the context's
// side -- the tables' upload, the one mask build per set, the apply launch in front of the nucleus filter; wh_op_constraint_mask / _apply (ops_debug.hip) are the
// kernels alone. tests/constraint_ref.py restates both in plain Python.
#include "kernels.h"

namespace wh
{
	namespace
	{
		// a transition entry as the kernels read it: a state of the automaton, or -1 for everything else (tables that are nobody's DFA cost wrong bits, never a fault)
		__device__ __forceinline__ int conEntry( int x, int nStates ) { return (unsigned)x < (unsigned)nStates ? x : -1; }
		// token t's bytes as [ off, off + len ) held inside tokBytes [nBytes], len at most CON_MAX_TOKEN_BYTES
		__device__ __forceinline__ void conTokenSpan( const ConstraintTables& t, int tok, long long& off, int& len )
		{
			const long long a = min( max( (long long)t.tokOffsets[ tok ], 0ll ), t.nBytes ), b = (long long)t.tokOffsets[ tok + 1 ];
			off = a;
			len = (int)min( min( max( b - a, 0ll ), (long long)CON_MAX_TOKEN_BYTES ), t.nBytes - a );
		}

		// ---- the mask: allowed[ s ][ t / 32 ] bit t % 32 = walk( s, t ) survives, for every state s and text token t < eot. Once per set. ----------------------
		// nStates x eot walks of a few bytes each -- 2 * 10^8 at the limits -- and every step of a walk is one dependent table lookup, so the table is where it is
		// cheapest to look up and every lane keeps several walks in flight:
		//   workgroup  1024 threads = 16 waves = 1024 consecutive tokens ( blockIdx.x ) x one tile of up to CM_TILE states ( blockIdx.y ). It stages the WHOLE
		//              transition table in LDS once, as int16 (a state is below 4096, -1 = none): at the limit 65536 entries = 128 KB of gfx950's 160 KB, next to
		//              classOf (256 B) and the tile's output words (16 KB). One workgroup per CU, 4 waves per SIMD.
		//   wave       64 consecutive token ids. Per state, ONE ballot of "my walk survived" is the two u32 words of the line for those 64 tokens.
		//   lane       its token's first 16 bytes, already mapped to classes, packed in four registers for the whole tile; a longer token (rare: the vocabulary's
		//              mean is about 7 bytes) reloads its further bytes in chunks of 16, only while one of the lane's walks is still alive. The lane walks its
		//              token from CM_GROUP = 4 states at a time: four independent chains of ds_read_u16 hide each other's latency.
		//   stores     the ballots go to LDS [state][32 words]; behind the tile the workgroup writes them out, 32 consecutive lanes one state's 32 words: a wave
		//              stores two whole 128-byte runs per instruction instead of 16 waves storing 8 bytes each. Plain vector stores, no atomics: every word of
		//              [nStates][nWords] has exactly one writer.
		// A token at or behind eot (the last workgroup's tail) and a token of zero bytes are dead from every state: their bits are 0. A word at or behind nWords
		// and a state at or behind nStates are computed as zeros and never stored.
		constexpr int CM_THREADS = 1024, CM_WAVES = CM_THREADS / 64, CM_WORDS = CM_THREADS / 32, CM_TILE = 128, CM_GROUP = 4, CM_REG_BYTES = 16;
		constexpr size_t cmLdsBytes( int tile, int entries ) { return (size_t)tile * CM_WORDS * 4 + ( ( (size_t)entries * 2 + 3 ) & ~(size_t)3 ) + 256; }
		static_assert( cmLdsBytes( CM_TILE, CON_MAX_ENTRIES ) <= 160 * 1024, "constraintMaskKernel LDS" );

		__device__ __forceinline__ void cmWalk16( const short* __restrict__ tr, int nClasses, const unsigned ( &w )[ 4 ], int n, int ( &cur )[ CM_GROUP ] )
		{
#pragma unroll
			for( int i = 0; i < CM_REG_BYTES; i++ )
			{
				if( i >= n ) break;
				const int cls = (int)( ( w[ i >> 2 ] >> ( 8 * ( i & 3 ) ) ) & 255u );
#pragma unroll
				for( int k = 0; k < CM_GROUP; k++ )
				{
					const int nxt = tr[ max( cur[ k ], 0 ) * nClasses + cls ];
					cur[ k ] = cur[ k ] < 0 ? -1 : nxt;
				}
			}
		}

		__global__ void __launch_bounds__( CM_THREADS ) constraintMaskKernel( const ConstraintTables t, int eot, unsigned* __restrict__ allowed, int tile )
		{
			extern __shared__ unsigned cmLds[];
			const int entries = t.nStates * t.nClasses;
			unsigned* const out = cmLds;																   // [tile][CM_WORDS]
			short* const tr = (short*)( out + tile * CM_WORDS );										   // [nStates][nClasses]
			unsigned char* const cls = (unsigned char*)tr + ( ( (size_t)entries * 2 + 3 ) & ~(size_t)3 );   // [256]
			const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
			for( int i = tid; i < entries; i += CM_THREADS ) tr[ i ] = (short)conEntry( t.trans[ i ], t.nStates );
			if( tid < 256 ) cls[ tid ] = (unsigned char)min( (int)t.classOf[ tid ], t.nClasses - 1 );
			__syncthreads();

			const int tok = (int)blockIdx.x * CM_THREADS + tid;
			const bool waveHasTokens = (int)blockIdx.x * CM_THREADS + wave * 64 < eot;	  // wave-uniform
			long long off = 0;
			int len = 0;
			if( tok < eot ) conTokenSpan( t, tok, off, len );
			unsigned w0[ 4 ] = { 0u, 0u, 0u, 0u };
#pragma unroll
			for( int i = 0; i < CM_REG_BYTES; i++ )
				if( i < len ) w0[ i >> 2 ] |= (unsigned)cls[ t.tokBytes[ off + i ] ] << ( 8 * ( i & 3 ) );
			const int n0 = min( len, CM_REG_BYTES );

			const int sBase = (int)blockIdx.y * tile;
			for( int g = 0; g < tile; g += CM_GROUP )
			{
				int cur[ CM_GROUP ];
#pragma unroll
				for( int k = 0; k < CM_GROUP; k++ ) cur[ k ] = ( len > 0 && g + k < tile && sBase + g + k < t.nStates ) ? sBase + g + k : -1;
				if( waveHasTokens )
				{
					cmWalk16( tr, t.nClasses, w0, n0, cur );
					// the bytes behind the registers' 16: reloaded, while the token goes on and one of this lane's walks is alive
					// (the loop's trip count is the wave's: every lane reaches the vote, and at most 16 chunks hold 255 bytes)
					for( int at = CM_REG_BYTES; at <= CON_MAX_TOKEN_BYTES; at += CM_REG_BYTES )
					{
						const bool mine = at < len && ( cur[ 0 ] >= 0 || cur[ 1 ] >= 0 || cur[ 2 ] >= 0 || cur[ 3 ] >= 0 );
						if( !__any( mine ) ) break;
						if( mine )
						{
							const int n = min( len - at, CM_REG_BYTES );
							unsigned w[ 4 ] = { 0u, 0u, 0u, 0u };
#pragma unroll
							for( int i = 0; i < CM_REG_BYTES; i++ )
								if( i < n ) w[ i >> 2 ] |= (unsigned)cls[ t.tokBytes[ off + at + i ] ] << ( 8 * ( i & 3 ) );
							cmWalk16( tr, t.nClasses, w, n, cur );
						}
					}
				}
#pragma unroll
				for( int k = 0; k < CM_GROUP; k++ )
				{
					const unsigned long long alive = __ballot( cur[ k ] >= 0 );
					if( lane == 0 && g + k < tile )
					{
						out[ ( g + k ) * CM_WORDS + wave * 2 ] = (unsigned)alive;
						out[ ( g + k ) * CM_WORDS + wave * 2 + 1 ] = (unsigned)( alive >> 32 );
					}
				}
			}
			__syncthreads();
			for( int i = tid; i < tile * CM_WORDS; i += CM_THREADS )
			{
				const int s = sBase + ( i / CM_WORDS ), word = (int)blockIdx.x * CM_WORDS + ( i % CM_WORDS );
				if( s < t.nStates && word < t.nWords ) allowed[ (long long)s * t.nWords + word ] = out[ i ];
			}
		}

		// ---- the step: advance each row's state over the token it sampled last, then penalise what the new state does not allow. One launch per step. ----------
		// One workgroup of 256 threads per row. Thread 0 alone advances the state: the walk is a chain of at most 255 dependent loads from the tables in global
		// memory (L2-resident: every row of every step reads the same few KB), far too short to share; the new state reaches the others through LDS.
		// The state's line of `allowed` -- 6.5 KB at the medium vocabulary -- is staged in LDS with 128-bit loads (the line starts at s * nWords words, so the words
		// in front of the first 16-byte boundary and behind the last go one by one), and the logits row is streamed in 128-bit accesses peeled to ITS alignment
		// the same way (a row starts at row * nVocab floats and nVocab is odd): the four bits of a float4 come from two neighbouring LDS words, because the row's
		// alignment and the line's are unrelated. A float4 whose four columns are all allowed is not stored. A dead row (-1) stages no line: every bit is 0.
		// x - penalty: -inf stays -inf, and with penalty = +inf every finite entry becomes -inf. Column eot is thread 0's, behind the loop that never reaches it.
		// Every thread reads the state and the fed token, the barrier follows, and only then thread 0 writes the state back: no lane can see the new one.
		constexpr int CA_THREADS = 256, CA_LINE_WORDS = CON_MAX_VOCAB / 32;

		__device__ int caAdvance( const ConstraintTables& t, int s, int tok, int eot )
		{
			if( s == CON_STATE_ARMED ) return t.start;
			if( tok < 0 || tok >= eot || s < 0 ) return s;
			long long off;
			int len;
			conTokenSpan( t, tok, off, len );
			if( len == 0 ) return -1;
			for( int i = 0; i < len && s >= 0; i++ )
			{
				const int cls = min( (int)t.classOf[ t.tokBytes[ off + i ] ], t.nClasses - 1 );
				s = conEntry( t.trans[ s * t.nClasses + cls ], t.nStates );
			}
			return s;
		}

		__global__ void __launch_bounds__( CA_THREADS ) constraintApplyKernel( float* __restrict__ logits, int nVocab, int eot, const ConstraintTables* __restrict__ tablesDev,
			const ConstraintTables byValue, const int* __restrict__ fed, int reset, int* __restrict__ states )
		{
			__shared__ unsigned line[ CA_LINE_WORDS + 1 ];
			__shared__ int newState;
			ConstraintTables t = tablesDev ? *tablesDev : byValue;
			t.nStates = min( max( t.nStates, 1 ), CON_MAX_STATES );
			t.nClasses = min( max( t.nClasses, 1 ), CON_MAX_CLASSES );
			t.start = min( max( t.start, 0 ), t.nStates - 1 );
			const int row = blockIdx.x, tid = (int)threadIdx.x;
			if( reset )
			{
				if( tid == 0 ) states[ row ] = reset == 2 ? CON_STATE_ARMED : t.start;
				return;
			}
			const int old = min( max( states[ row ], CON_STATE_ARMED ), t.nStates - 1 );
			const int tok = fed[ row ];
			__syncthreads();
			if( tid == 0 )
			{
				newState = caAdvance( t, old, tok, eot );
				states[ row ] = newState;
			}
			__syncthreads();
			const int s = newState;
			const int lim = min( eot, nVocab ), nWords = min( ( lim + 31 ) >> 5, min( t.nWords, CA_LINE_WORDS ) );
			if( s >= 0 )
			{
				const unsigned* const src = t.allowed + (long long)s * t.nWords;
				const int head = min( (int)( ( 4u - ( (unsigned)( (size_t)src >> 2 ) & 3u ) ) & 3u ), nWords ), body = ( nWords - head ) >> 2;
				if( tid < head ) line[ tid ] = src[ tid ];
				for( int i = tid; i < body; i += CA_THREADS )
				{
					const uint4 v = *(const uint4*)( src + head + 4 * i );
					line[ head + 4 * i ] = v.x; line[ head + 4 * i + 1 ] = v.y; line[ head + 4 * i + 2 ] = v.z; line[ head + 4 * i + 3 ] = v.w;
				}
				for( int i = head + 4 * body + tid; i < nWords; i += CA_THREADS ) line[ i ] = src[ i ];
			}
			else
				for( int i = tid; i < nWords; i += CA_THREADS ) line[ i ] = 0u;
			// columns the line does not cover (tables built for a smaller eot than this launch's) count as forbidden, like a dead row's
			for( int i = nWords + tid; i <= min( ( lim + 31 ) >> 5, CA_LINE_WORDS ); i += CA_THREADS ) line[ i ] = 0u;
			__syncthreads();
			const float penalty = t.penalty;
			float* const x = logits + (long long)row * nVocab;
			const auto bitsAt = [ & ]( int c ) -> unsigned	// the bits of columns c .. c + 3 (c + 31 may reach into the word behind: line has one more)
			{
				const unsigned long long two = (unsigned long long)line[ c >> 5 ] | ( (unsigned long long)line[ ( c >> 5 ) + 1 ] << 32 );
				return (unsigned)( two >> ( c & 31 ) ) & 15u;
			};
			const int head = min( (int)( ( 4u - ( (unsigned)( (size_t)x >> 2 ) & 3u ) ) & 3u ), lim ), body = ( lim - head ) >> 2;
			if( tid < head && !( bitsAt( tid ) & 1u ) ) x[ tid ] = x[ tid ] - penalty;
			for( int i = tid; i < body; i += CA_THREADS )
			{
				const int c = head + 4 * i;
				const unsigned b = bitsAt( c );
				if( b == 15u ) continue;
				float4 v = *(const float4*)( x + c );
				if( !( b & 1u ) ) v.x = v.x - penalty;
				if( !( b & 2u ) ) v.y = v.y - penalty;
				if( !( b & 4u ) ) v.z = v.z - penalty;
				if( !( b & 8u ) ) v.w = v.w - penalty;
				*(float4*)( x + c ) = v;
			}
			for( int c = head + 4 * body + tid; c < lim; c += CA_THREADS )
				if( !( bitsAt( c ) & 1u ) ) x[ c ] = x[ c ] - penalty;
			if( tid == 0 && eot < nVocab && s >= 0 && !t.accept[ s ] ) x[ eot ] = x[ eot ] - penalty;
		}
	}	// namespace

	int launchConstraintMask( const ConstraintTables& t, int eot, unsigned* allowed, hipStream_t stream )
	{
		if( !t.classOf || !t.trans || !t.tokOffsets || !t.tokBytes || !allowed || eot < 1 || eot > CON_MAX_VOCAB || t.nStates < 1 || t.nStates > CON_MAX_STATES || t.nClasses < 1 ||
			t.nClasses > CON_MAX_CLASSES || t.nStates * t.nClasses > CON_MAX_ENTRIES || t.nWords != ( eot + 31 ) / 32 || t.nBytes < 0 )
		{
			setError( "constraintMask: bad argument" );
			return -1;
		}
		// the tile of states: as large as CM_TILE (the table is staged once per workgroup), halved while the grid would leave most of the chip idle
		const int blocksX = ( eot + CM_THREADS - 1 ) / CM_THREADS;
		int tile = CM_TILE;
		while( tile > 8 && blocksX * ( ( t.nStates + tile - 1 ) / tile ) < 512 && tile / 2 >= CM_GROUP ) tile /= 2;
		const dim3 grid( (unsigned)blocksX, (unsigned)( ( t.nStates + tile - 1 ) / tile ) );
		return launchLds<constraintMaskKernel, (int)cmLdsBytes( CM_TILE, CON_MAX_ENTRIES )>( grid, dim3( CM_THREADS ), cmLdsBytes( tile, t.nStates * t.nClasses ), stream, t, eot, allowed, tile );
	}

	int launchConstraintApply( float* logits, int rows, int nVocab, int eot, const ConstraintTables* tablesDev, const ConstraintTables& t, const int* fed, int reset, int* states,
		hipStream_t stream )
	{
		if( !logits || !states || ( !reset && !fed ) || rows < 1 || nVocab < 1 || eot < 1 || eot > CON_MAX_VOCAB || eot > nVocab || reset < 0 || reset > 2 ||
			( !tablesDev && ( !t.classOf || !t.trans || !t.accept || !t.tokOffsets || !t.tokBytes || !t.allowed || t.nWords < 1 || t.nBytes < 0 ) ) )
		{
			setError( "constraintApply: bad argument" );
			return -1;
		}
		hipLaunchKernelGGL( constraintApplyKernel, dim3( rows ), dim3( CA_THREADS ), 0, stream, logits, nVocab, eot, tablesDev, t, fed, reset, states );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}	// namespace wh
