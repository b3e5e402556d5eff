// Top-k and nucleus (top-p) sampling (wh_context_set_nucleus; DESIGN.md section 7 "Top-k and nucleus sampling"): the kernel and its launch. filters.hip owns the
// context's side and launches it last of the decode-step logit filters; wh_op_nucleus_logits (ops_debug.hip) is the kernel alone.
#include "kernels.h"
#include <type_traits>

namespace wh
{
	namespace
	{
		// ---- keep a prefix of a row in the order ( value descending, id ascending ), -inf over the rest (restated in float64 by tests/nucleus_ref.py) ----
		// top_k: the prefix of k entries; a row with k or fewer entries above -inf is left alone. top_p < 1: of what top_k left, the shortest prefix whose share of
		// sum exp( ( x - max ) * invT ) reaches top_p, never empty. -inf and NaN are nobody's entry: never counted, never written. A row whose factor invT is not above
		// 0, or whose `on` word is 0, is a greedy row: the workgroup leaves before it reads anything.
		// One 1024-thread workgroup per row and ONE read of the row, peeled to 16-byte alignment as in topLogprobsKernel: 13 float4 per thread plus one scalar, kept in
		// registers as order-preserving 32-bit words (0 = no entry). An entry's KEY is 48 bits, ( ordered value << 16 ) | ( 65535 - id ): keys are unique, the larger key
		// is the larger value and, among equal values, the lower id -- so ties need no case of their own: the descent simply goes on into the id bits.
		// Selection is an MSB-first radix descent over the key in digits of 11, 11, 10 (the value), 11 and 5 bits (the id), one LDS histogram of up to 2048 buckets per
		// level: every entry that shares the prefix chosen so far adds itself to its digit's bucket, the workgroup scans the buckets from the top (two per thread:
		// shuffles in the wave, 16 wave totals through LDS) and the one thread whose bucket the target falls into publishes it. The result is a FLOOR: kept = key >= floor.
		//   top_k  buckets count entries, the target is k. The descent ends as soon as the chosen bucket is kept whole -- with distinct values around the cut, at level 3.
		//   top_p  buckets also carry mass, over the entries at or above top_k's floor only, and the target is top_p x the total, which the first level's scan gives.
		//          The descent ends when the chosen bucket holds one entry: the one at which the running mass reaches the target, kept.
		// Mass is exact and its sum has NO order: e = expf( ( x - max ) * invT ) -- single precision, an FP32 argument -- is in [0, 1] with 24 significant bits, and
		// e * 2^47 is added as a 64-bit integer (ds_add_u64). 53248 entries stay below 2^63, what an entry loses is below 2^-48 of the largest term, and integer
		// addition is associative, so the LDS atomics may land in any order: the same row gives the same bits on every launch. (A sum in double through atomics
		// would not; one in a fixed order needs the entries of a bucket sorted.) The target is ceil( double( top_p ) * total ), held to [ 1, total ].
		// The first level is the expensive one: all 53 entries of every thread go to the histogram, and logits crowd into a few dozen of its buckets, so lanes of a
		// wave meet on one LDS address. It runs once -- by count when top_k is on (top_p then walks the k survivors), by mass when top_p stands alone. Later levels
		// touch the handful of entries under the prefix.
		// Write-back: -inf to the entries below the floor and to nothing else; a float4 whose four entries all go leaves as one 16-byte store.
		// Resource usage on gfx950 and the measurement: profiles/nucleus_resources.txt, profiles/nucleus_probe.json. The 128 registers without scratch rest on the
		// empty asm statements and the scalar moves below, which a compiler is free to see differently: after a toolchain change run
		// `python tools/kernel_resources.py nucleus.hip` and hold it against that file.
		constexpr int NUC_THREADS = 1024, NUC_VEC = 13, NUC_BUCKETS = 2048, NUC_LEVELS = 5;
		static_assert( NUC_VEC * 4 * NUC_THREADS == NUCLEUS_MAX_VOCAB && NUCLEUS_MAX_VOCAB <= 65536, "the row in registers, the id in 16 bits" );
		static_assert( NUC_BUCKETS == 2 * NUC_THREADS, "the scan owns two buckets per thread" );
		using u64 = unsigned long long;

		struct NucShared
		{
			u64 mass[ NUC_BUCKETS ];
			unsigned cnt[ NUC_BUCKETS ];
			u64 waveTotal[ 16 ];
			unsigned waveMax[ 16 ];
			u64 foundAbove;			  // what the buckets above the chosen one hold
			unsigned foundBucket, foundCnt;
		};

		__device__ __forceinline__ unsigned nucOrd( float v )
		{
			if( !( v > -INFINITY ) ) return 0u;		  // -inf and NaN
			unsigned b = __float_as_uint( v );
			if( b == 0x80000000u ) b = 0u;			  // -0 is 0: one value, ordered by id
			return ( b & 0x80000000u ) ? ~b : ( b | 0x80000000u );
		}
		__device__ __forceinline__ float nucValue( unsigned ord ) { return __uint_as_float( ( ord & 0x80000000u ) ? ( ord ^ 0x80000000u ) : ~ord ); }
		// a key, or the floor of a kept set, as its two halves; below = the smaller key
		struct NucFloor { unsigned ord, id; };
		__device__ __forceinline__ bool nucBelow( unsigned ord, unsigned inv, NucFloor f ) { return ord < f.ord || ( ord == f.ord && inv < f.id ); }
		__device__ __forceinline__ int nucShift( int level ) { return level == 0 ? 37 : level == 1 ? 26 : level == 2 ? 16 : level == 3 ? 5 : 0; }
		__device__ __forceinline__ int nucBits( int level ) { return level == 2 ? 10 : level == 4 ? 5 : 11; }
		// a value every lane holds alike, moved to a scalar register: what comes out of LDS or device memory is a vector register's until the compiler is told
		__device__ __forceinline__ unsigned nucUniform( unsigned v ) { return (unsigned)__builtin_amdgcn_readfirstlane( (int)v ); }
		__device__ __forceinline__ u64 nucUniform( u64 v ) { return ( (u64)nucUniform( (unsigned)( v >> 32 ) ) << 32 ) | nucUniform( (unsigned)v ); }
		// e * 2^47 as an integer; the row maximum itself, or +inf against +inf, is 1
		__device__ __forceinline__ u64 nucMass( unsigned ord, float m, float invT )
		{
			const float d = nucValue( ord ) - m;
			const float e = d == d ? expf( d * invT ) : 1.0f;
			return (u64)( e * 140737488355328.0f );
		}

		// The bucket the target falls into, scanning nb buckets from the top: MASS ? sh.mass : sh.cnt. frac > 0: the target becomes ceil( frac * total ) in [ 1, total ].
		// Every thread returns the total and the target; sh.found* hold the bucket when 1 <= target <= total. Ends with a barrier.
		template<bool MASS>
		__device__ __forceinline__ void nucFind( NucShared& sh, int nb, double frac, u64& target, u64& total )
		{
			const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
			const int b0 = nb - 1 - 2 * t, b1 = b0 - 1;
			u64 a0 = 0, a1 = 0;
			if( b0 >= 0 ) a0 = MASS ? sh.mass[ b0 ] : (u64)sh.cnt[ b0 ];
			if( b1 >= 0 ) a1 = MASS ? sh.mass[ b1 ] : (u64)sh.cnt[ b1 ];
			u64 incl = a0 + a1;
#pragma unroll
			for( int o = 1; o < 64; o <<= 1 )
			{
				const u64 y = __shfl_up( incl, o, 64 );
				if( lane >= o ) incl += y;
			}
			if( lane == 63 ) sh.waveTotal[ wave ] = incl;
			__syncthreads();
			u64 base = 0;
			total = 0;
#pragma unroll
			for( int i = 0; i < 16; i++ )
			{
				const u64 w = sh.waveTotal[ i ];
				if( i < wave ) base += w;
				total += w;
			}
			if( frac > 0.0 )
			{
				target = (u64)ceil( frac * (double)total );
				target = target < 1 ? 1 : target > total ? total : target;
			}
			total = nucUniform( total );
			target = nucUniform( target );
			const u64 e0 = base + incl - ( a0 + a1 ), i0 = e0 + a0, i1 = i0 + a1;
			if( a0 && e0 < target && target <= i0 ) { sh.foundBucket = (unsigned)b0; sh.foundAbove = e0; sh.foundCnt = sh.cnt[ b0 ]; }
			if( a1 && i0 < target && target <= i1 ) { sh.foundBucket = (unsigned)b1; sh.foundAbove = i0; sh.foundCnt = sh.cnt[ b1 ]; }
			__syncthreads();
		}

		__global__ void __launch_bounds__( NUC_THREADS ) nucleusLogitsKernel( float* __restrict__ logits, long long rowStride, int nVocab, const NucleusParams* __restrict__ prm,
			int topK, float topP, const float* __restrict__ invTDev, int invTStride, const unsigned* __restrict__ onDev, int onStride )
		{
			__shared__ NucShared sh;
			const int t = threadIdx.x, row = blockIdx.x;
			const float invT = __uint_as_float( nucUniform( __float_as_uint( invTDev[ (long long)row * invTStride ] ) ) );
			if( !( invT > 0.0f ) || ( onDev && onDev[ (long long)row * onStride ] == 0u ) ) return;
			if( prm ) { topK = (int)nucUniform( (unsigned)prm->topK ); topP = __uint_as_float( nucUniform( __float_as_uint( prm->topP ) ) ); }
			const bool byMass = topP < 1.0f;
			if( topK <= 0 && !byMass ) return;

			float* const x = logits + (long long)row * rowStride;
			const int head = min( (int)( ( 4u - ( (unsigned)( (size_t)x >> 2 ) & 3u ) ) & 3u ), nVocab );
			const int nVec = ( nVocab - head ) >> 2;
			const int tail0 = head + 4 * nVec;
			float4* const xv = (float4*)( x + head );
			float4 v[ NUC_VEC ];
#pragma unroll
			for( int i = 0; i < NUC_VEC; i++ )
			{
				const int j = t + NUC_THREADS * i;
				v[ i ] = make_float4( -INFINITY, -INFINITY, -INFINITY, -INFINITY );
				if( j < nVec ) v[ i ] = xv[ j ];
			}
			int extraId = -1;
			if( t < head ) extraId = t;
			else if( t >= 4 && tail0 + ( t - 4 ) < nVocab ) extraId = tail0 + ( t - 4 );
			unsigned extra = 0u;
			if( extraId >= 0 ) extra = nucOrd( x[ extraId ] );
			// slot 4 * i + j of thread t is element id0 + 4096 * i + j
			unsigned key[ 4 * NUC_VEC ];
			unsigned best = extra;
#pragma unroll
			for( int i = 0; i < NUC_VEC; i++ )
			{
				key[ 4 * i ] = nucOrd( v[ i ].x );
				key[ 4 * i + 1 ] = nucOrd( v[ i ].y );
				key[ 4 * i + 2 ] = nucOrd( v[ i ].z );
				key[ 4 * i + 3 ] = nucOrd( v[ i ].w );
				best = max( max( best, max( key[ 4 * i ], key[ 4 * i + 1 ] ) ), max( key[ 4 * i + 2 ], key[ 4 * i + 3 ] ) );
			}
			const int id0 = head + 4 * t;
			// Every pass forms the ids again and takes the entries through an empty asm the compiler cannot see through. Without it everything that does not depend on
			// the level -- 53 ids, 53 values, 53 masses of 64 bits -- is hoisted out of the level loop and spilled.
			const auto eachEntry = [ & ]( auto&& f )
			{
				int base = id0;
				asm volatile( "" : "+v"( base ) );
#pragma unroll
				for( int s = 0; s < 4 * NUC_VEC; s++ )
				{
					asm volatile( "" : "+v"( key[ s ] ) );
					f( key[ s ], base + ( s >> 2 ) * ( 4 * NUC_THREADS ) + ( s & 3 ) );
				}
				asm volatile( "" : "+v"( extra ) );
				f( extra, extraId );
			};

			// the row maximum: the mass is relative to it
#pragma unroll
			for( int o = 32; o > 0; o >>= 1 ) best = max( best, (unsigned)__shfl_xor( (int)best, o, 64 ) );
			if( ( t & 63 ) == 0 ) sh.waveMax[ t >> 6 ] = best;
			__syncthreads();
			best = sh.waveMax[ t & 15 ];
#pragma unroll
			for( int o = 8; o > 0; o >>= 1 ) best = max( best, (unsigned)__shfl_xor( (int)best, o, 64 ) );
			best = nucUniform( best );
			if( best == 0u ) return;		  // no entry in the row
			const float m = nucValue( best );

			// One descent: the floor of the prefix that holds `target` entries (MASS false) or reaches frac of the mass (true) among the entries at or above `keep`.
			// A key is handled as its two halves, the value word and 65535 - id: the value word is the register the entry lives in, nothing 64 bits wide is formed
			const auto descend = [ & ]( auto massTag, u64 target, double frac, NucFloor keep ) -> NucFloor
			{
				constexpr bool MASS = decltype( massTag )::value;
				NucFloor prefix = { 0u, 0u };
				for( int level = 0; level < NUC_LEVELS; level++ )
				{
					const bool byId = level >= 3;
					const int bits = nucBits( level ), shift = byId ? nucShift( level ) : nucShift( level ) - 16, up = shift + bits;
					const unsigned mask = ( 1u << bits ) - 1u, above = up >= 32 ? 0u : ~0u << up, want = byId ? prefix.id : prefix.ord;
					for( int b = t; b < NUC_BUCKETS; b += NUC_THREADS ) { sh.cnt[ b ] = 0u; sh.mass[ b ] = 0ull; }
					__syncthreads();
					eachEntry( [ & ]( unsigned ord, int id )
					{
						if( !ord ) return;
						const unsigned inv = 0xFFFFu - (unsigned)id;
						if( nucBelow( ord, inv, keep ) || ( byId && ord != prefix.ord ) ) return;
						const unsigned src = byId ? inv : ord;
						if( ( src ^ want ) & above ) return;
						const unsigned d = ( src >> shift ) & mask;
						atomicAdd( &sh.cnt[ d ], 1u );
						if constexpr( MASS ) atomicAdd( &sh.mass[ d ], nucMass( ord, m, invT ) );
					} );
					__syncthreads();
					u64 total;
					nucFind<MASS>( sh, 1 << bits, level == 0 ? frac : 0.0, target, total );
					// fewer entries than asked for, or no mass at all: everything at or above `keep` stays
					if( level == 0 && ( total == 0 || ( !MASS && total <= target ) ) ) return keep;
					const unsigned bucket = nucUniform( sh.foundBucket ), held = nucUniform( sh.foundCnt );
					if( byId ) prefix.id |= bucket << shift;
					else prefix.ord |= bucket << shift;
					target -= nucUniform( sh.foundAbove );
					if( MASS ? held == 1u : target == (u64)held ) break;
				}
				return nucBelow( prefix.ord, prefix.id, keep ) ? keep : prefix;
			};
			NucFloor floor = { 0u, 0u };
			if( topK > 0 ) floor = descend( std::false_type(), (u64)topK, 0.0, floor );
			if( byMass ) floor = descend( std::true_type(), 0ull, (double)topP, floor );
			if( floor.ord == 0u ) return;		  // every entry stays

			// (the store addresses are formed from the thread index again, not kept from the loads)
			int wt = t;
			asm volatile( "" : "+v"( wt ) );
#pragma unroll
			for( int i = 0; i < NUC_VEC; i++ )
			{
				const int id = head + 4 * wt + i * ( 4 * NUC_THREADS );
				bool go[ 4 ];
#pragma unroll
				for( int j = 0; j < 4; j++ ) go[ j ] = key[ 4 * i + j ] != 0u && nucBelow( key[ 4 * i + j ], 0xFFFFu - (unsigned)( id + j ), floor );
				if( go[ 0 ] && go[ 1 ] && go[ 2 ] && go[ 3 ] ) xv[ wt + NUC_THREADS * i ] = make_float4( -INFINITY, -INFINITY, -INFINITY, -INFINITY );
				else
				{
#pragma unroll
					for( int j = 0; j < 4; j++ )
						if( go[ j ] ) x[ id + j ] = -INFINITY;
				}
			}
			if( extra != 0u && nucBelow( extra, 0xFFFFu - (unsigned)extraId, floor ) ) x[ extraId ] = -INFINITY;
		}
	}	// namespace

	int launchNucleusLogits( float* logits, long long rowStride, int rows, int nVocab, const NucleusParams* prmDev, int topK, float topP, const float* invTDev, int invTStride,
		const unsigned* onDev, int onStride, hipStream_t stream )
	{
		if( !logits || !invTDev || rows < 1 || nVocab < 1 || nVocab > NUCLEUS_MAX_VOCAB || rowStride < nVocab || invTStride < 0 || onStride < 0 ||
			( !prmDev && ( topK < 0 || topK > NUCLEUS_MAX_K || !( topP > 0.0f && topP <= 1.0f ) ) ) )
		{
			setError( "nucleusLogits: bad argument" );
			return -1;
		}
		hipLaunchKernelGGL( nucleusLogitsKernel, dim3( rows ), dim3( NUC_THREADS ), 0, stream, logits, rowStride, nVocab, prmDev, topK, topP, invTDev, invTStride, onDev, onStride );
		WH_HIP( hipGetLastError() );
		return 0;
	}
}	// namespace wh
